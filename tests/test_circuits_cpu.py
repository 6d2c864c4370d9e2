"""Circuit-level parity on the CPU (no GPU): this repo's circuit library
(peba1_amd/csrc/circuits.cpp) versus the reference's src/Math.cpp, both run over the
plaintext-bit provider of the tfhe API (tests/mock).  Same values, same gate counts and
the same gate sequence (hash of every call with its operands).  The golden file was
produced by the reference's own code (tests/refcompat/make_golden.sh)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "circuit_known_answers.json")


def ref_built(name):
    """A program build() compiled from the reference's unmodified sources into oracle/_ref/ (oracle/Makefile `ref`, run
    where those sources exist at build time)."""
    path = os.path.join(ROOT, "oracle", "_ref", name)
    if not os.path.exists(path):
        pytest.skip(f"oracle/_ref/{name} not built (build() compiles it where the reference sources exist)")
    return path


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    t = str(tmp_path_factory.mktemp("refcompat"))
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=gnu++11", "-fPIC", "-shared", "-I" + inc,
                           os.path.join(ROOT, "tests/mock/plain_tfhe.cpp"), "-o", t + "/libplain_tfhe.so"])
    # this repo's circuits, compiled from source against the mock (no HIP needed)
    subprocess.check_call(["g++", "-O1", "-std=gnu++17", "-I" + inc,
                           os.path.join(ROOT, "tests/refcompat/driver.cpp"),
                           os.path.join(ROOT, "peba1_amd/csrc/circuits.cpp"), os.path.join(ROOT, "peba1_amd/csrc/circuits_fast.cpp"),
                           "-o", t + "/driver_mine", "-L" + t, "-lplain_tfhe", "-Wl,-rpath," + t])
    return t


def run(path):
    return json.loads(subprocess.check_output([path]).decode())


def test_circuits_match_golden(built):
    mine = run(built + "/driver_mine")
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert mine == golden


def test_golden_holds_survey_known_answers():
    """SURVEY.md 8c table (obtained there by running the reference over a mock)."""
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["addn8_122_204"]["value"] == 70 + 256                    # 70, carry 1
    assert (g["addn8_122_204"]["xor"], g["addn8_122_204"]["and"]) == (32, 24)
    assert g["twosc8_5"]["value"] == 251
    assert g["subn8_122_204"]["value"] == 82
    assert (g["subn8_122_204"]["xor"], g["subn8_122_204"]["and"], g["subn8_122_204"]["or"],
            g["subn8_122_204"]["not"]) == (121, 96, 9, 9)
    assert g["mult8_122_204"]["value"] == 24888
    assert (g["mult8_122_204"]["xor"], g["mult8_122_204"]["and"]) == (704, 592)
    # bootsABS on 9-bit two's-complement numbers (main.cpp:374) and the shift helpers (Math.cpp:183-211):
    # values AND gate sequence (the trace hash, compared by test_circuits_match_golden) from the reference
    assert (g["abs9_minus82"]["value"], g["abs9_plus77"]["value"]) == (82, 77)
    assert g["abs9_minus82"]["blind_rotates"] == 72 and g["abs9_minus82"]["copy"] == 37
    assert (g["shl8_b5_by3"]["value"], g["shr8_b5_by3"]["value"], g["shlnr8_b5_by2"]["value"]) == (0xA8, 0x16, 0xD4)
    assert g["shl8_b5_by3"]["blind_rotates"] == 0 and g["shlnr8_b5_by2"]["copy"] == 14
    assert g["euclid128_genuine"]["value"] == 128
    assert g["euclid128_impostor"]["value"] == 1400950
    e = g["euclid128_impostor"]
    assert (e["xor"], e["and"], e["or"], e["not"], e["copy"], e["const"]) == (117376, 96896, 1152, 1152, 120704, 16640)
    for k, want in [("function_f_genuine_bound0", 1), ("function_f_impostor_bound0", 1),
                    ("function_f_genuine_bound256", 0), ("function_f_impostor_bound256", 1)]:
        assert g[k]["value"] == want                                   # (distance > bound), SURVEY D2
        assert g[k]["blind_rotates"] == 215544 and g[k]["mux"] == 48 and g[k]["xnor"] == 24


def test_reference_sources_compile_against_our_headers_and_agree(built):
    """Drop-in proof: the reference's unmodified Math.cpp builds against include/tfhe/*.h and,
    over the same provider, issues exactly the gate sequence our circuits issue."""
    assert run(ref_built("driver_ref_mock")) == run(built + "/driver_mine")


def test_reference_main_and_client_compile_against_our_headers():
    """src/main.cpp and src/Client.cpp compile unmodified (needs <vector> via tfhe_io.h)."""
    for obj, symbol in (("main.o", "main"), ("Client.o", None)):
        syms = subprocess.check_output(["nm", "--defined-only", ref_built(obj)]).decode().split()
        assert syms and (symbol is None or symbol in syms), obj


def test_reference_program_golden_output_is_current():
    """tests/golden/reference_main_output.txt is what the reference's own program prints over the
    plaintext-bit provider with time() fixed (tests/refcompat/make_golden_main.sh): regenerate and
    compare, so the file the GPU test checks against cannot go stale.  The run itself shows the
    reference's defects at work: a zero template byte makes its own
    Euclidean self-check print 65152 instead of 128, Manhattan prints 126, and the protocol still
    'authenticates'."""
    out = subprocess.check_output([ref_built("main_mock")]).decode()
    # the lines make_golden_main.sh leaves out: they report durations
    got = "".join(l for l in out.splitlines(keepends=True) if not re.search(r"seconds|Function [fg]( bitwise)?: ", l))
    with open(os.path.join(ROOT, "tests", "golden", "reference_main_output.txt")) as g:
        want = g.read()
    assert got == want
    for line in ("Addition: 128 success, 0 fails", "Multiplication: 128 success, 0 fails",
                 "The result for Euclidean distance is 65152 and should be 128", "Client 7 successfully authenticated to the server!"):
        assert line in want
