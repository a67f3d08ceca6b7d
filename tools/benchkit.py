"""What the tools/bench_*.py share: the interleaved timing loop."""


def timed_interleaved(ctx, candidates, reps, rounds, warmup=3):
    """{name: fn} -> {name: median / min / max ms per call}: every round times each candidate once, in turn
    (`reps` calls between two events); each candidate runs `warmup` times before the first round."""
    import libsdr_amd as sa   # (the caller has put the repository root on sys.path; some import the package late)
    for fn in candidates.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in candidates}
    for _ in range(rounds):
        for k, fn in candidates.items():
            t = sa.Timer(ctx)
            t.start()
            for _ in range(reps):
                fn()
            t.stop()
            ms[k].append(t.elapsed_ms() / reps)
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = {"ms": round(v[len(v) // 2], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5)}
    return out
