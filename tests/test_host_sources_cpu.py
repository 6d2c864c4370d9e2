"""Every host file that shim.cpp includes into its object parses on its own.

build.sh compiles shim.cpp as one translation unit (it is one of the files kernels_sha16 hashes, so a new host source is
not named there lightly); the files included at shim.cpp's end each state what they use, through shim_internal.hpp and
their own #include lines.  Here each of them goes through build.sh's host compiler, with build.sh's HOSTFLAGS, alone: a
file that leans on what happens to stand above it in shim.cpp does not parse.  No GPU, no library.
"""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "peba1_amd", "csrc")
SOURCES = ("pack_host.cpp", "unpack_host.cpp", "select_host.cpp", "compressed_host.cpp", "seeded_host.cpp",
           "seeded_lwe_host.cpp", "test_entries.cpp", "recorder.cpp")


def host_compile_line():
    """(compiler, flags) exactly as build.sh sets them: its own assignments, evaluated by the shell it runs under."""
    with open(os.path.join(CSRC, "build.sh")) as f:
        assigns = [ln for ln in f.read().splitlines() if re.match(r"(ROCM|CXX|FLAGS|HOSTFLAGS)=", ln)]
    assert [ln.split("=")[0] for ln in assigns] == ["ROCM", "CXX", "FLAGS", "HOSTFLAGS"], assigns
    out = subprocess.check_output(["bash", "-euc", "\n".join(assigns) + '\nprintf "%s\\n%s\\n" "$CXX" "$HOSTFLAGS"'], text=True)
    cxx, flags = out.splitlines()
    return cxx, flags.split()


def test_shim_includes_exactly_these_files():
    with open(os.path.join(CSRC, "shim.cpp")) as f:
        included = re.findall(r'^#include "(\w+\.cpp)"', f.read(), re.M)
    assert sorted(included) == sorted(SOURCES)


def test_each_included_host_file_parses_on_its_own():
    cxx, flags = host_compile_line()
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip(f"the host compiler of build.sh is absent: {cxx}")

    def parse(name):
        return name, subprocess.run([cxx, *flags, "-fsyntax-only", name], cwd=CSRC, capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=8) as pool:
        runs = list(pool.map(parse, SOURCES))
    failed = {name: run.stderr[-2000:] for name, run in runs if run.returncode != 0}
    assert not failed, "\n".join(f"{name} does not parse on its own:\n{err}" for name, err in failed.items())
