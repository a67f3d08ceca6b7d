"""The existing kernels of the channelizer family before and after the real-input form, on one device in one session: runs
tools/bench_channelizer.py, tools/bench_chanaudio.py and tools/bench_chanpower.py as child processes, alternating the PARENT
commit's library and this tree's (SDRHIP_LIB, the A/B hook of libsdr_amd/abi.py), `passes` times each, and merges every
candidate's [median, min, max] ms per call into profiles/chanreal_bench.json under family_parent_vs_this, with whether this
tree's medians lie inside (or below) the parent's own range over its passes.
The parent's library: check the parent commit out into a directory of its own, `make -C libsdr_amd/csrc` there, and pass the
path of its libsdr_amd/libsdrhip.so.
usage: python tools/bench_chanreal_family.py <parent libsdrhip.so> [reps] [rounds] [passes] [out.json]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ("channelizer", "chanaudio", "chanpower")


def stages(result):
    """{candidate: {ms, min_ms, max_ms}} of a bench tool's json (bench_chanaudio.py nests them per shape)"""
    if "stages" in result:
        return result["stages"]
    out = {}
    for shape, part in result.get("shapes", {}).items():
        for k, v in (part.get("stages", {}) if isinstance(part, dict) else {}).items():
            out[shape + "_" + k] = v
    return out


def main():
    parent = os.path.abspath(sys.argv[1])
    reps, rounds, passes = (sys.argv[2:5] + ["20", "7", "2"][len(sys.argv[2:5]):])
    out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "chanreal_bench.json")
    this = os.path.join(ROOT, "libsdr_amd", "libsdrhip.so")
    runs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tool in TOOLS:
            rows = {}
            for p in range(int(passes)):
                for side, lib in (("parent", parent), ("this", this)):
                    path = os.path.join(tmp, "%s_%s_%d.json" % (tool, side, p))
                    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_%s.py" % tool), reps, rounds, path], check=True,
                                   env=dict(os.environ, SDRHIP_LIB=lib), stdout=subprocess.DEVNULL, timeout=600)
                    with open(path) as f:
                        for k, v in stages(json.load(f)).items():
                            if isinstance(v, dict) and "ms" in v:
                                rows.setdefault(k, {"parent": [], "this": []})[side].append([v["ms"], v["min_ms"], v["max_ms"]])
            for k, row in rows.items():
                hi = max(v[2] for v in row["parent"])
                row["this_medians_within_or_below_parent_range"] = max(v[0] for v in row["this"]) <= hi
                print("%s %s: parent %s this %s%s" % (tool, k, [v[0] for v in row["parent"]], [v[0] for v in row["this"]],
                                                      "" if row["this_medians_within_or_below_parent_range"] else "  ABOVE the parent's range"), flush=True)
            runs[tool] = rows
    result = {}
    if os.path.exists(out):
        with open(out) as f:
            result = json.load(f)
    result["family_parent_vs_this"] = {"reps": int(reps), "rounds": int(rounds), "passes": int(passes),
                                       "note": "per candidate and side, one [median, min, max] ms per call per pass; the sides alternate",
                                       "runs": runs}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
