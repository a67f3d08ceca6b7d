"""TEST CODE shared by tests/test_cpp_pocsag_assemble.py and tests/test_cpp_pocsag.py: the golden POCSAG cases as the text file
the C++ programs read (the format is described in tests/cpp/pocsag_cases.hh). Events come from the restatement, run in the
recorded call splits; deliveries, messages, scores and the numeric reading are the reference's own record
(tests/golden/manifest_pocsag.json); the text reading is libsdr_amd.pocsag.Message's."""
import json
import os

import numpy as np

import pocsag_restatement as P
from libsdr_amd.pocsag import Message

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest_pocsag.json")))


def _hex(b):
    return bytes(b).hex() or "-"


def write_cases(path):
    """-> (cases, messages) written"""
    man = manifest()
    bits = np.fromfile(os.path.join(GOLDEN, man["bits"]["file"]), np.uint8)
    lines, n_msgs = [], 0
    for c in man["cases"]:
        lines.append("c %s" % c["name"])
        dec, at, deliveries = P.Decoder(), c["offset"], iter(c["deliveries"])
        for k, n in enumerate(c["splits"]):
            for word, info in dec.process(bits[at:at + n]):
                lines.append("e %d %d" % (word, info))
                if info & 3 == P.END:
                    call, msgs = next(deliveries)
                    assert call == k, (c["name"], call, k)
                    lines.append("d %d" % call)
                    for a, f, nb, payload, est_text, est_num, numeric in msgs:
                        m = Message(a, f)
                        m.bits, m.payload = nb, bytearray.fromhex(payload)
                        lines.append("m %d %d %d %s %d %d %s %s" % (a, f, nb, payload or "-", est_text, est_num, _hex(numeric.encode()),
                                                                    _hex(m.as_text().encode("latin-1"))))
                        n_msgs += 1
            at += n
        assert next(deliveries, None) is None, c["name"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(man["cases"]), n_msgs
