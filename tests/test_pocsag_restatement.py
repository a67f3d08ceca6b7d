"""The POCSAG restatement (tests/pocsag_restatement.py) and the host-side message assembly (libsdr_amd.pocsag) against the
fixtures cut from the unmodified reference (tools/golden_pocsag -> tests/golden/g19_pocsag_*, manifest_pocsag.json), and the two
rules the device code rests on — the syndrome table and the popcount sync test — against pocsag_repair's search. No GPU."""
import json
import os

import numpy as np
import pytest

import pocsag_restatement as P
from libsdr_amd.pocsag import Message, MessageAssembler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAN = json.load(open(os.path.join(GOLDEN, "manifest_pocsag.json")))
BITS = np.fromfile(os.path.join(GOLDEN, MAN["bits"]["file"]), np.uint8)
CASES = {c["name"]: c for c in MAN["cases"]}
ADDRESS_WORD = P.address_word((0x2345 << 3) | 2, 3)


def case_bits(c):
    return BITS[c["offset"]:c["offset"] + c["n"]]


def windows(bits):
    """every 32-bit window a node sees while it reads `bits` from a zero register"""
    v, out = 0, []
    for b in bits.tolist():
        v = ((v << 1) | (b & 1)) & 0xFFFFFFFF
        out.append(v)
    return out


def search_repair_for(bits):
    """pocsag_repair by SEARCH, evaluated once for every window of the row (one vectorised pass) and looked up per bit"""
    w = np.array(sorted(set(windows(bits))), np.uint32)
    rc, out = P.repair_search_many(w)
    memo = {int(a): (int(r), int(o)) for a, r, o in zip(w, rc, out)}
    return lambda word: memo[word]


def run_case(c, repair):
    """-> (states after every call, deliveries [(call, [message keys])], events per call)"""
    bits, dec, asm = case_bits(c), P.Decoder(repair), MessageAssembler(1)
    states, deliveries, per_call, at = [], [], [], 0
    for k, n in enumerate(c["splits"]):
        ev = dec.process(bits[at:at + n])
        at += n
        per_call.append(ev)
        states.append(dec.state())
        for msgs in asm.feed_row(0, np.array(ev, np.uint32).reshape(-1, 2)):
            deliveries.append((k, [m.key() for m in msgs]))
    return states, deliveries, per_call


def golden_states(c):
    return [(s, b, sl, int(h, 16)) for s, b, sl, h in c["states"]]


def golden_deliveries(c):
    return [(k, [(m[0], m[1], m[2], bytes.fromhex(m[3])) for m in msgs]) for k, msgs in c["deliveries"]]


def test_the_fixtures_hold_the_cases_the_decoder_is_specified_by():
    want = {"clean", "clean_ragged", "data_1", "data_2", "addr_1", "addr_2", "sync_1", "sync_2", "data_3_dropped", "sync_3_missed", "cont_sync_2",
            "cont_sync_3_end", "cut_mid_batch", "noise", "sync_one_bit_after_end", "data_without_address", "sync_inside_batch", "upper_bits_set"}
    assert want <= set(CASES)
    assert all(sum(c["splits"]) == c["n"] for c in CASES.values())
    assert CASES["noise"]["n"] == 4096 and MAN["messages"] > 20
    assert (case_bits(CASES["upper_bits_set"]) >= 0xFE).all()
    # what each case is there for, read off the reference's own record
    both = golden_deliveries(CASES["clean"])[0][1]
    assert [m[:3] for m in both] == [((0x2345 << 3) | 2, 3, 120), ((0x777 << 3) | 1, 0, 80)]
    for name in ("data_1", "data_2", "addr_1", "addr_2", "sync_1", "sync_2", "cont_sync_2", "upper_bits_set", "clean_ragged"):
        assert [m for _, ms in golden_deliveries(CASES[name]) for m in ms] == both, name
    assert [m[2] for _, ms in golden_deliveries(CASES["data_3_dropped"]) for m in ms] == [100, 80]
    assert [m[0] for _, ms in golden_deliveries(CASES["sync_3_missed"]) for m in ms] == [(0x777 << 3) | 1]
    assert [m[0] for _, ms in golden_deliveries(CASES["cont_sync_3_end"]) for m in ms] == [(0x2345 << 3) | 2]
    assert golden_deliveries(CASES["cut_mid_batch"]) == [] and golden_states(CASES["cut_mid_batch"])[-1][0] == P.RECEIVE
    assert golden_deliveries(CASES["noise"]) == []
    late = golden_deliveries(CASES["sync_one_bit_after_end"])
    assert len(late) == 2 and late[0][0] == 0 and late[1][1][0][0] == (0x777 << 3) | 1
    assert golden_states(CASES["sync_one_bit_after_end"])[:2] == [(P.WAIT, 32, 8, golden_states(CASES["sync_one_bit_after_end"])[0][3]),
                                                                 (P.RECEIVE, 0, 0, golden_states(CASES["sync_one_bit_after_end"])[1][3])]
    assert golden_deliveries(CASES["data_without_address"]) == [(1, [])]
    inside = golden_deliveries(CASES["sync_inside_batch"])[0][1]
    assert [m[:3] for m in inside] == [((((P.SYNC_WORD >> 13) & 0x3FFFF) << 3) | 1, (P.SYNC_WORD >> 11) & 3, 20)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_states_and_messages_match_the_reference(name):
    c = CASES[name]
    states, deliveries, per_call = run_case(c, search_repair_for(case_bits(c)))
    assert states == golden_states(c)
    assert deliveries == golden_deliveries(c)
    # the table rule drives the same machine to the same events
    assert run_case(c, P.repair_table) == (states, deliveries, per_call)
    for n, ev in zip(c["splits"], per_call):
        assert len(ev) <= P.out_capacity(n), (n, len(ev))
        assert [i >> 8 for _, i in ev] == sorted(i >> 8 for _, i in ev) and all((i >> 8) < n for _, i in ev)


def test_repair_matches_the_reference_list():
    w = np.fromfile(os.path.join(GOLDEN, MAN["repair_in"]["file"]), np.uint32)
    want = np.fromfile(os.path.join(GOLDEN, MAN["repair_out"]["file"]), np.uint32).reshape(-1, 2)
    assert w.size == want.shape[0] > 3000 and 0 < want[:, 0].sum() < w.size
    rc, out = P.repair_search_many(w)
    assert np.array_equal(rc, want[:, 0]) and np.array_equal(out, want[:, 1])
    for k in (0, 1, 2, 17, 500, w.size - 1):   # the one-word form
        assert P.repair_search(int(w[k])) == (int(want[k, 0]), int(want[k, 1]))


def test_syndrome_forms_agree_and_the_encoder_makes_codewords():
    r = np.random.default_rng(5).integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
    assert [P.syndrome(int(v)) for v in r] == P.syndrome_np(r).tolist()
    assert P.codeword(P.SYNC_WORD >> 11) == P.SYNC_WORD and P.codeword(P.IDLE_WORD >> 11) == P.IDLE_WORD
    assert all(P.syndrome(P.codeword(d)) == 0 for d in (0, 1, 0x1FFFFF, 0x155555, 0x0ABCDE))
    assert (P.TABLE >= 0).sum() == 529 and sorted(bin(int(e)).count("1") for e in P.TABLE[P.TABLE >= 0]) == [0] + [1] * 32 + [2] * 496


def _rule_words():
    w = np.fromfile(os.path.join(GOLDEN, MAN["repair_in"]["file"]), np.uint32).tolist()
    for base in (P.SYNC_WORD, P.IDLE_WORD, ADDRESS_WORD):
        c = P.corruptions(base, 3)
        assert len(c) == 1 + 32 + 496 + 4960   # the 6545 multisets of up to three flips are these distinct words
        w += c
    w += np.random.default_rng(0x90C5A6).integers(0, 1 << 32, 100000, dtype=np.uint64).tolist()
    return np.array(w, np.uint32)


def test_table_rule_and_popcount_rule_equal_the_search():
    w = _rule_words()
    rc, out = P.repair_search_many(w)
    trc, tout = P.repair_table_many(w)
    assert np.array_equal(rc, trc) and np.array_equal(out, tout)
    sync_by_repair = (rc == 0) & (out == P.SYNC_WORD)
    pop = np.array([bin(int(v) ^ P.SYNC_WORD).count("1") for v in w]) <= 2
    assert np.array_equal(sync_by_repair, pop) and 500 < pop.sum() < 600
    for k in range(0, w.size, 997):   # the scalar forms
        assert P.repair_table(int(w[k])) == (int(rc[k]), int(out[k])) and P.is_sync_popcount(int(w[k])) == bool(pop[k])


def test_event_count_never_exceeds_the_capacity():
    # back-to-back valid batches, no preamble between them: the densest event stream there is
    rng = np.random.default_rng(3)
    batch = [P.codeword(int(d)) for d in rng.integers(0, 1 << 21, 16)]
    bits = np.concatenate([np.array(P.word_bits(w), np.uint8) for _ in range(12) for w in [P.SYNC_WORD] + batch])
    dec = P.Decoder()
    assert len(dec.process(bits)) == 1 + 12 * 16 <= P.out_capacity(bits.size)
    for step in (1, 31, 32, 33, 63, 64, 65, 100, 543, 544, 545, 2048):
        dec, at = P.Decoder(), 0
        while at < bits.size:
            n = min(step, bits.size - at)
            assert len(dec.process(bits[at:at + n])) <= P.out_capacity(n), (step, at)
            at += n
    # one bit, entered at bit count 63 with two codewords in the register: both WORD events at bit 0
    for slot in (0, 7):
        dec = P.Decoder()
        both = (batch[0] << 32) | batch[1]
        dec.st, dec.bitcount, dec.slot, dec.shift = P.RECEIVE, 63, slot, both >> 1
        ev = dec.process(np.array([both & 1], np.uint8))
        assert ev == [(batch[0], P.WORD | (slot << 2)), (batch[1], P.WORD | (slot << 2))] and len(ev) <= P.out_capacity(1)
        assert dec.state()[:3] == ((P.RECEIVE, 0, 1) if slot == 0 else (P.CHECK_CONTINUE, 0, 8))


def test_message_text_and_numbers():
    text, num = [Message(a, f) for a, f, _, _ in golden_deliveries(CASES["clean"])[0][1]]
    for m, words in ((text, P.text_words("HELLO POCSAG 42")), (num, P.numeric_words("0123456789-[]U ."))):
        for w in words:
            m.add_payload(w)
    assert [m.key() for m in (text, num)] == golden_deliveries(CASES["clean"])[0][1]
    assert text.as_text() == "HELLO POCSAG 42<NUL><NUL>" and num.as_numeric() == "0123456789-[]U .    "
    assert text.estimate_text() == 15 - 2 * 5 and num.estimate_numeric() > num.estimate_text()
    # every message the reference delivered, any case: its two scores and its numeric reading
    seen = 0
    for c in CASES.values():
        for _, msgs in c["deliveries"]:
            for a, f, nb, payload, est_text, est_num, numeric in msgs:
                m = Message(a, f)
                m.bits, m.payload = nb, bytearray.fromhex(payload)
                assert (m.estimate_text(), m.estimate_numeric(), m.as_numeric()) == (est_text, est_num, numeric), (c["name"], m)
                seen += 1
    assert seen == MAN["messages"]
    assert Message(5, 1).as_text() == "" and Message(5, 1).bits == 0
