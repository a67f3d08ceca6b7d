"""Device-resident timing of the split FFT filter (FilterSink -> FilterSource, sdrhip_fftsink / sdrhip_fftsource) beside the
single-band fused overlap-add plan (sdrhip_fftconv, FFTCONV_OLA) on the same input. Stages are timed with HIP events over
`reps` calls after warm-up; the share of 8 TB/s counts 24 B per input sample per stage (forward: 8 read + 16 written,
inverse: 16 read + 8 written). Run under `rocprofv3 --kernel-trace --stats -- python tools/time_filter_split.py` for the
per-kernel split. usage: python tools/time_filter_split.py [reps]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import libsdr_amd as sa

FS = 2.4e6
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
CASES = [(1024, 1024, 64), (8192, 64, 16)]   # (N, channels, blocks per channel), complex<float>


def timed(ctx, fn, reps):
    for _ in range(3):
        fn()
    t = sa.Timer(ctx)
    t.start()
    for _ in range(reps):
        fn()
    t.stop()
    return t.elapsed_ms() / reps


def main():
    ctx = sa.Context(0)
    rows = []
    for N, C, nb in CASES:
        n = N * nb
        K = sa.design_fftfilt_spectrum(sa.design_fftfilt_kernel(N, 50e3, 150e3, FS))
        x = np.random.default_rng(1).standard_normal((C, n, 2)).astype(np.float32)
        din, dspec, dout = ctx.malloc(x.nbytes), ctx.malloc(2 * x.nbytes), ctx.malloc(x.nbytes)
        try:
            ctx.h2d(din, x)
            sink = sa.FFTSink(ctx, N, channels=C, max_blocks=nb)
            src = sa.FFTSource(ctx, N, K, channels=C, max_blocks=nb)
            fused = sa.FFTConv(ctx, sa.FFTCONV_OLA, 2 * N, K, channels=C, max_in=n)
            t_fwd = timed(ctx, lambda: sink.process_dev(din, n, n, dspec, 2 * n), REPS)
            t_inv = timed(ctx, lambda: src.process_dev(dspec, nb, 2 * n, dout, n), REPS)
            t_chain = timed(ctx, lambda: (sink.process_dev(din, n, n, dspec, 2 * n), src.process_dev(dspec, nb, 2 * n, dout, n)), REPS)
            t_ola = timed(ctx, lambda: fused.process_dev(din, n, n, dout, n), REPS)
        finally:
            for p in (din, dspec, dout):
                ctx.free(p)
        samples = C * n
        roof_ms = samples * 24 / 8e12 * 1e3
        row = {"N": N, "channels": C, "blocks": nb, "form": sink.form, "forward_ms": round(t_fwd, 4), "inverse_ms": round(t_inv, 4),
               "forward_roofline_share": round(roof_ms / t_fwd, 3), "inverse_roofline_share": round(roof_ms / t_inv, 3),
               "chain_ms": round(t_chain, 4), "fftconv_ola_ms": round(t_ola, 4), "chain_over_ola": round(t_chain / t_ola, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    return rows


if __name__ == "__main__":
    main()
