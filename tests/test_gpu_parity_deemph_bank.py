"""GPU parity of the per-channel FMDeemph<int16_t> (sdrhip_deemphbank_i16_create, include/sdrhip_rx.h): every row of a bank
against the oracle's FMDeemph<int16_t> run on that row alone where the row is enabled, against its own input where it is not.
Bit for bit: there is no tolerance. The module name makes tests/conftest.py run every process() call inside the red-zoned
device arena (strided rows at every alignment, guard bands checked after every call).

70 rows cross the 64-lane workgroup of the one-lane form and leave the last workgroup of the speculative form (256 lanes =
64 ... 8 rows) ragged. The lengths walk the rows' head (< 8 samples), whole 16-byte chunks and tail, and both sides of the plan
rule of sdrhip_deemph::plan (lanes are split once a segment is as long as the run-in of 16 alpha samples in whole groups of 64):
alpha = 2 runs the one-lane form up to 17 samples and the speculative form at 255, 700 and 4096, alpha = 10 speculates at 4096
only (from 768 on; 700 is still one lane), alpha = 40 never, alpha = 1 copies."""
import ctypes as C
import os

import numpy as np
import pytest

import libsdr_amd as sa
from libsdr_amd import abi_rx

pytestmark = pytest.mark.gpu

ROWS = 70
LENS = [0, 1, 7, 8, 9, 15, 16, 17, 255, 700, 4096]
FLIP = {4: (5, 64, 69), 8: (5, 64, 69)}     # before the call of this index, these rows' flags are inverted
IRREGULAR = [bool((c * 7 + c // 5) % 3) and c not in (0, 63) or c in (1, 2, 64) for c in range(ROWS)]
PATTERNS = {"irregular": IRREGULAR, "all_on": [True] * ROWS, "all_off": [False] * ROWS}


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rows():
    """Noise rows of several loudnesses; row 1 holds only +/-32767 (every difference wraps the int16), row 2 only zeros."""
    r = np.random.default_rng(20261019)
    n = sum(LENS) + 17
    x = np.rint(r.normal(0, 1, (ROWS, n)) * r.uniform(50, 20000, (ROWS, 1))).clip(-32768, 32767).astype(np.int16)
    x[1] = np.where(r.integers(0, 2, n) > 0, 32767, -32767)
    x[2] = 0
    x.setflags(write=False)
    return x


def _ref(orc, alpha):
    d = orc.FMDeemphI16(22050.0)
    d.alpha = alpha
    return d


def _expect(refs, flags, x):
    return np.stack([refs[c].process(x[c]) if flags[c] else x[c] for c in range(ROWS)]) if x.shape[1] else np.zeros_like(x)


@pytest.mark.parametrize("alpha", [1, 2, 10, 40])
def test_bank_rows_vs_oracle(ctx, orc, rows, alpha, redzone):
    assert redzone == "redzone"
    assert sum(IRREGULAR) not in (0, ROWS) and IRREGULAR[1] and IRREGULAR[2] and not IRREGULAR[0]
    from redzone import RedZone
    calls0, ran = RedZone.calls, set()
    for name, pattern in PATTERNS.items():
        flags = list(pattern)
        node = sa.FMDeemphBankI16(ctx, alpha, flags, max_in=max(LENS))
        assert node.enabled() == flags
        refs = [_ref(orc, alpha) for _ in range(ROWS)]
        at = 0
        for k, n in enumerate(LENS):
            for c in FLIP.get(k, ()):
                flags[c] = not flags[c]
                node.set_enabled(c, flags[c])
            x = rows[:, at:at + n]
            at += n
            if n:
                ran.update(node.kernel_names(n))
            got = node.process(x)
            want = _expect(refs, flags, x)
            assert got.shape == want.shape and np.array_equal(got, want), (alpha, name, k, n, np.argwhere(got != want)[:4])
        assert node.enabled() == flags
        # reset: every average zero, the flags kept — a disabled row's average too (it is enabled afterwards and starts from 0)
        node.reset()
        assert node.enabled() == flags
        for c in (5, 0):
            flags[c] = True
            node.set_enabled(c, True)
        refs = [_ref(orc, alpha) for _ in range(ROWS)]
        x = rows[:, at:at + 17]
        got = node.process(x)
        assert np.array_equal(got, _expect(refs, flags, x)), (alpha, name, "after reset")
        node.close()
    assert RedZone.calls - calls0 == 3 * (len(LENS) - 1 + 1)
    want = {1: {"deemphbank_i16_copy_kernel"}, 2: {"deemphbank_i16_seq_kernel", "deemphbank_i16_spec_kernel"},
            10: {"deemphbank_i16_seq_kernel", "deemphbank_i16_spec_kernel"}, 40: {"deemphbank_i16_seq_kernel"}}[alpha]
    assert ran == want, ran


def test_plan_rule_and_kernel_names(ctx):
    """The bank answers with its own instances' names and follows the one-parameter handle's plan rule length for length."""
    for alpha in (1, 2, 10, 40):
        bank = sa.FMDeemphBankI16(ctx, alpha, [c % 2 == 0 for c in range(ROWS)], max_in=4096)
        one = sa.FMDeemphI16(ctx, alpha, channels=ROWS, max_in=4096)
        for n in [n for n in LENS if n] + [256, 767, 768]:
            a, b = bank.kernel_names(n), one.kernel_names(n)
            assert a == [b[0].replace("deemph_i16_", "deemphbank_i16_")], (alpha, n, a, b)
        bank.close()
        one.close()
    bank = sa.FMDeemphBankI16(ctx, 2, [True, False], max_in=4096)
    assert bank.kernel_names(17) == ["deemphbank_i16_seq_kernel"]
    assert bank.kernel_names(256) == bank.kernel_names() == ["deemphbank_i16_spec_kernel"]   # a mixed bank speculates
    bank.close()
    b10, b40 = sa.FMDeemphBankI16(ctx, 10, [True, False], max_in=4096), sa.FMDeemphBankI16(ctx, 40, [True, False], max_in=4096)
    assert b10.kernel_names(700) == ["deemphbank_i16_seq_kernel"] and b10.kernel_names(768) == ["deemphbank_i16_spec_kernel"]
    assert b40.kernel_names(4096) == ["deemphbank_i16_seq_kernel"]
    b10.close()
    b40.close()


def test_handle_types_and_channel_range(ctx):
    L = abi_rx.lib()
    one = sa.FMDeemphI16(ctx, 2, channels=3, max_in=64)
    e = (C.c_int * 3)()
    assert L.sdrhip_deemphbank_i16_set_enabled(one._h, 0, 0) == sa.abi.E_UNSUPPORTED
    assert L.sdrhip_deemphbank_i16_get_enabled(one._h, e, 3) == sa.abi.E_UNSUPPORTED
    one.close()
    bank = sa.FMDeemphBankI16(ctx, 2, [True, False, True], max_in=64)
    for c in (-1, 3):
        assert L.sdrhip_deemphbank_i16_set_enabled(bank._h, c, 1) == sa.abi.E_INVALID
        assert "outside [0,3)" in L.sdrhip_last_error().decode()
    assert L.sdrhip_deemphbank_i16_get_enabled(bank._h, e, 2) == sa.abi.E_SIZE
    assert bank.enabled() == [True, False, True]
    bank.close()


def test_a_stale_runtime_error_is_not_blamed_on_the_launch(ctx, orc):
    """The HIP runtime keeps the last error of ANY call of the thread until somebody asks for it, and a launch can only be
    checked by asking. An error an unrelated call left behind — here hipSetDevice with an ordinal that does not exist, called
    on the runtime directly; in a long-lived process a handle that outlived its context, or another library's failed query —
    must not make the next de-emphasis call fail, on either kind of handle."""
    names = sorted({os.path.basename(line.split()[-1]) for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert names, "the library's HIP runtime is not mapped"
    hip = C.CDLL(names[0])                       # (already loaded: the same runtime instance the library calls)
    x = np.arange(2 * 40, dtype=np.int16).reshape(2, 40) * 100
    bank, one = sa.FMDeemphBankI16(ctx, 2, [True, False], max_in=64), sa.FMDeemphI16(ctx, 2, channels=2, max_in=64)
    want = _ref(orc, 2).process(x[0])
    for node in (bank, one):
        assert hip.hipSetDevice(1 << 20) != 0    # hipErrorInvalidDevice, now the thread's last error
        got = node.process(x)
        assert np.array_equal(got[0], want)
    assert np.array_equal(got[1], _ref(orc, 2).process(x[1]))
    bank.close()
    one.close()
