"""How the tests build a C++ program: one g++ line, one place for its flags, and a build counts only if it is free of
warnings. Programs live in tests/cpp (or `srcdir`), executables go to tests/_build."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror=return-type", "-I" + os.path.join(ROOT, "include")]
LINK = ["-L" + os.path.join(ROOT, "libsdr_amd"), "-lsdrhip", "-Wl,-rpath," + os.path.join(ROOT, "libsdr_amd")]
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build(program, extra_flags=(), link=True, out=None, srcdir=("tests", "cpp"), cxx=CXX):
    """program (a file of srcdir) -> the path of its executable `out` (default: the program's name without .cc). link: against
    libsdrhip.so; a program that needs other libraries names them in extra_flags. cxx: the compiler and its base flags."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, out or os.path.splitext(program)[0])
    cmd = list(cxx) + [os.path.join(ROOT, *srcdir, program), "-o", exe] + list(extra_flags) + (LINK if link else []) + ["-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe
