"""Second half of `make golden`: adds to tests/golden/manifest_psk31.json what the cut tool cannot know — the figures of this
library against the fixtures it just wrote. "designer": the worst error of sdrhip_design_inpol_taps and of the reference's table,
rows 0 ... 64, on a complex tone at 0.1 cycles per sample. "defined_sincos": with the defined sincos in place of the C library's,
whether every fixture's bits and counts are the same (a condition on the fixtures: choose other signals if not) and the largest
deviation of P, F, mu, omega from the reference's state after any call (recorded, no bar). Needs libsdrhip.so built.
usage: python tools/golden_psk31/annotate.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libsdr_amd as sa
import psk31_restatement as R


def tone_error(tab, rows):
    w, k = 2 * np.pi * 0.1, np.arange(8) - 4
    return float(max(abs(np.sum(tab[r].astype(np.float64) * np.exp(1j * w * k)) - np.exp(-1j * w * r / 128.0)) for r in rows))


def main():
    path = os.path.join(R.GOLDEN, "manifest_psk31.json")
    m = json.load(open(path))
    m["designer"] = {"tone_cycles_per_sample": 0.1, "rows": "0...64", "designed_worst_error": tone_error(sa.design_inpol_taps(), range(65)),
                     "reference_worst_error": tone_error(R.table(), range(65))}
    same, dev, row128 = True, {}, 0
    for Fs in sorted({m[n]["Fs"] for n in R.fixture_names()}):
        names = [n for n in R.fixture_names() if m[n]["Fs"] == Fs]
        fx = [R.fixture(n) for n in names]
        lens = fx[0][0]["lens"]
        bank = R.Bank(Fs, [f[0]["dF"] for f in fx], R.table())
        x = np.stack([f[1].astype(np.float32) for f in fx])
        off, got, worst = 0, [[] for _ in fx], 0.0
        for b, L in enumerate(lens):
            out = bank.process(x[:, off:off + L])
            off += L
            st = bank.state()
            for k, f in enumerate(fx):
                got[k].append(out[k])
                same &= len(out[k]) == f[0]["counts"][b]
                a = st[k][:4].astype(np.uint32).view(np.float32)
                w = np.array(f[0]["state_bits"][b][:4], np.uint32).view(np.float32)
                worst = max(worst, float(np.max(np.abs(a - w))))
        for k, f in enumerate(fx):
            same &= bool(np.array_equal(np.concatenate(got[k]), f[2]))
        dev["%g" % Fs] = worst
        row128 += bank.row128
    m["defined_sincos"] = {"bits_and_counts_identical": bool(same), "largest_state_deviation_by_sample_rate": dev, "row128_sub_samples": row128}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in m.items()) + "\n}\n")
    print(json.dumps({k: m[k] for k in ("designer", "defined_sincos")}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
