#!/usr/bin/env python3
"""Per-kernel digests of device assembly (hipcc -S --cuda-device-only output), to show that a host-side change leaves
every kernel's code as it was.

usage: tools/isa_digest.py file.s ... > digests.txt     then diff two such files (parent build, change).

A kernel's digest covers its instructions from its label to .Lfunc_endN and its .amdhsa_kernel block, with ';' comments
dropped and .L labels renumbered by first use. Each output line: digest, how many times the kernel was compiled, its name.
"""
import collections
import hashlib
import re
import sys

LABEL = re.compile(r"\.L[\w$.]+")


def kernels(text):
    lines = text.splitlines()
    meta = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            meta[m.group(1)] = lines[i:j + 1]
    for i, l in enumerate(lines):
        m = re.match(r"^([\w$.]+):", l)
        if not m or m.group(1) not in meta:
            continue
        j = i
        while not lines[j].startswith(".Lfunc_end"):
            j += 1
        yield m.group(1), lines[i:j] + meta[m.group(1)]


def digest(body):
    names = {}
    h = hashlib.sha256()
    for l in body:
        l = l.split(";", 1)[0].rstrip()
        if l:
            h.update(LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), l).encode() + b"\n")
    return h.hexdigest()[:16]


def main(paths):
    seen = collections.defaultdict(list)
    for p in paths:
        with open(p) as f:
            for name, body in kernels(f.read()):
                seen[name].append(digest(body))
    for name in sorted(seen):
        print(" ".join(sorted(set(seen[name]))), len(seen[name]), name)


if __name__ == "__main__":
    main(sys.argv[1:])
