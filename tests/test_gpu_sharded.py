"""GPU tests of the two multi-GPU configurations of BASELINE.json on the HIP path, with logical
ranks on the one device a test box has:
  configs[2]  one 256-slot x 8-bit match, slots partitioned over N ranks, 24-ciphertext partial
              sums exchanged, adder tree + comparator on rank 0 (peba1_amd/dist.py);
  configs[3]  1-to-N identification: independent matches streamed through the slot pool in
              bounded flushes (bench.py --mode identify runs the same loop at 128 per GPU).
Ciphertext parity of the sharded DAG against the oracle evaluating the same DAG:
tests/golden/sharded_match_digest.json (made by tests/golden/make_sharded_digest.py)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sharded_dag_ciphertexts_match_oracle_digest(p128_keys):
    """3 slots over 2 logical ranks (2 + 1): the packed partial sums each rank would put on the wire
    and the 24 output ciphertexts hash to what the CPU oracle produced through the same circuit
    library for the same DAG -- DESIGN.md section 8's claim, word for word."""
    import torch
    from peba1_amd import api, circuits, lib
    from peba1_amd import dist as pd
    pp, ks, _ = p128_keys
    with open(os.path.join(ROOT, "tests", "golden", "sharded_match_digest.json")) as f:
        g = json.load(f)
    assert g["key_seed"] == 0x5EBA2 and g["world"] == 2
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(g["encrypt_seed"])
    bits = g["bits"]
    T, S = [], []
    for t, s in zip(g["template"], g["probe"]):          # encryption order is part of the fixture
        T.append(circuits.encrypt_number(pp, t, bits, ks))
        S.append(circuits.encrypt_number(pp, s, bits, ks))
    bound = circuits.encrypt_number(pp, g["bound"], 3 * bits, ks)
    digests = {}

    def hook(rank, packed):
        digests[rank] = hashlib.sha256(packed.cpu().numpy().tobytes()).hexdigest()

    api.reset_stats()
    api.set_deferred(True)
    try:
        res = pd.sharded_match_logical(torch, L, circuits.load(), pp.ptr, ks.cloud, pp.words,
                                       [a.ptr for a in S], [a.ptr for a in T], bound.ptr, bits, g["world"],
                                       device="cuda", partial_hook=hook)
        api.flush()
    finally:
        api.set_deferred(False)
    st = api.stats()
    assert st["blind_rotates"] <= g["blind_rotates"] <= st["blind_rotates"] + 2 * (st["reused_gates"] + st["dead_gates"])
    assert [digests[r] for r in range(g["world"])] == g["partial_sha256"]
    res_ls = C.cast(res, lib.LS)
    words = np.zeros((24, pp.words), dtype=np.int32)
    assert L.tfhe_hip_export_samples(res_ls, 24, pp.ptr, words.ctypes.data_as(lib.I32P)) == 0
    assert hashlib.sha256(words[0].tobytes()).hexdigest() == g["result_b0_sha256"]
    assert hashlib.sha256(words.tobytes()).hexdigest() == g["result_b_sha256"]
    assert L.bootsSymDecrypt(res_ls, ks.ptr) == g["match_bit"]
    L.delete_gate_bootstrapping_ciphertext_array(24, res_ls)


def test_latency_form_of_the_sharded_match_ciphertexts_match_oracle_digest(p128_keys):
    """PEBA1_DIST_FAST_PARTIAL | PEBA1_DIST_FAST_COMBINE: every rank's slots through the depth-optimised distance circuit,
    the gather, the depth-optimised combine -- 5 slots over 2 logical ranks (3 + 2), both sides of the threshold.  Each
    rank's packed partial sum and both 24-ciphertext results hash to what the CPU oracle produced for the same DAG
    (tests/golden/make_sharded_digest.py --latency-form)."""
    import torch
    from peba1_amd import api, circuits, lib
    from peba1_amd import dist as pd
    pp, ks, _ = p128_keys
    with open(os.path.join(ROOT, "tests", "golden", "sharded_match_latency_form_digest.json")) as f:
        g = json.load(f)
    assert g["key_seed"] == 0x5EBA2
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(g["encrypt_seed"])
    bits, world = g["bits"], g["world"]
    T, S = [], []
    for t, s in zip(g["template"], g["probe"]):          # encryption order is part of the fixture
        T.append(circuits.encrypt_number(pp, t, bits, ks))
        S.append(circuits.encrypt_number(pp, s, bits, ks))
    bounds = [circuits.encrypt_number(pp, b, 3 * bits, ks) for b in g["bounds"]]
    api.set_deferred(True)
    try:
        parts = []
        for r in range(world):
            lo, hi = pd.shard_slots(len(T), world, r)
            parts.append(pd.local_partial_packed(ks.cloud, pp.words, [a.ptr for a in S[lo:hi]], [a.ptr for a in T[lo:hi]], bits, fast=True))
        results = [pd.combine_packed(L, pp.ptr, ks.cloud, parts, b.ptr, fast=True) for b in bounds]
        api.flush()
    finally:
        api.set_deferred(False)
    assert [hashlib.sha256(p.tobytes()).hexdigest() for p in parts] == g["partial_sha256"]
    tmp = api.CiphertextArray(pp, 24)
    for r in range(world):
        assert L.tfhe_hip_import_samples(tmp.ptr, 24, pp.ptr, np.ascontiguousarray(parts[r]).ctypes.data_as(lib.I32P)) == 0
        assert circuits.decrypt_number(tmp, ks) == g["partial_values"][r], r
    for res, want_sha, want_bit in zip(results, g["result_b_sha256"], g["match_bits"]):
        ls = C.cast(res, lib.LS)
        words = np.zeros((24, pp.words), dtype=np.int32)
        assert L.tfhe_hip_export_samples(ls, 24, pp.ptr, words.ctypes.data_as(lib.I32P)) == 0
        assert hashlib.sha256(words.tobytes()).hexdigest() == want_sha
        assert L.bootsSymDecrypt(ls, ks.ptr) == want_bit
        L.delete_gate_bootstrapping_ciphertext_array(24, ls)


def test_cfg3_256_slots_over_8_ranks_ciphertexts_match_oracle_digest(p128_keys):
    """BASELINE configs[2] at its own size, word for word: 256 slots x 8 bit (uniform bytes from the fixture's LCG)
    over 8 logical ranks of 32 slots.  Each rank's packed 24-ciphertext partial sum -- what crosses the exchange --
    and the 24 outputs of rank 0's combine, in both forms (ripple tree and carry-save / prefix), hash to what the CPU
    oracle produced evaluating the same 432k-rotation DAG (tests/golden/make_sharded_digest.py --slots256; the
    bound sits just under the distance, so the comparator's whole chain decides the bit)."""
    import torch
    from peba1_amd import api, circuits, lib
    from peba1_amd import dist as pd

    def synthetic_bytes(n, seed):                        # the generator's LCG (make_sharded_digest.synthetic_bytes)
        x, out = seed, []
        for _ in range(n):
            x = (x * 1103515245 + 12345) % (1 << 31)
            out.append((x >> 16) & 255)
        return out

    pp, ks, _ = p128_keys
    with open(os.path.join(ROOT, "tests", "golden", "sharded_match_256_digest.json")) as f:
        g = json.load(f)
    assert g["key_seed"] == 0x5EBA2 and g["world"] == 8 and g["nslots"] == 256
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(g["encrypt_seed"])
    bits = g["bits"]
    template = synthetic_bytes(g["nslots"], g["template_lcg_seed"])
    probe = [v or 1 for v in synthetic_bytes(g["nslots"], g["probe_lcg_seed"])]
    assert sum((a - b) ** 2 for a, b in zip(probe, template)) == g["distance"] == g["bound"] + 1
    T, S = [], []
    for t, s in zip(template, probe):                    # encryption order is part of the fixture
        T.append(circuits.encrypt_number(pp, t, bits, ks))
        S.append(circuits.encrypt_number(pp, s, bits, ks))
    bound = circuits.encrypt_number(pp, g["bound"], 3 * bits, ks)
    parts = {}
    api.reset_stats()
    api.set_deferred(True)
    try:
        res = pd.sharded_match_logical(torch, L, circuits.load(), pp.ptr, ks.cloud, pp.words,
                                       [a.ptr for a in S], [a.ptr for a in T], bound.ptr, bits, g["world"],
                                       device="cuda", partial_hook=lambda r, t: parts.__setitem__(r, t.numpy().copy()))
        api.flush()
        fast = pd.combine_packed(L, pp.ptr, ks.cloud, [parts[r] for r in range(g["world"])], bound.ptr, fast=True)
        api.flush()
    finally:
        api.set_deferred(False)
    st = api.stats()
    assert st["blind_rotates"] <= g["blind_rotates_recorded"]
    assert [hashlib.sha256(parts[r].tobytes()).hexdigest() for r in range(g["world"])] == g["partial_sha256"]
    tmp = api.CiphertextArray(pp, 24)
    for r in range(g["world"]):
        host = np.ascontiguousarray(parts[r])
        assert L.tfhe_hip_import_samples(tmp.ptr, 24, pp.ptr, host.ctypes.data_as(lib.I32P)) == 0
        assert circuits.decrypt_number(tmp, ks) == g["partial_values"][r], r
    for ptr, key in ((res, "result_b_sha256"), (fast, "result_b_fast_sha256")):
        ls = C.cast(ptr, lib.LS)
        words = np.zeros((24, pp.words), dtype=np.int32)
        assert L.tfhe_hip_export_samples(ls, 24, pp.ptr, words.ctypes.data_as(lib.I32P)) == 0
        assert hashlib.sha256(words.tobytes()).hexdigest() == g[key], key
        assert L.bootsSymDecrypt(ls, ks.ptr) == g["match_bit"] == 1
        L.delete_gate_bootstrapping_ciphertext_array(24, ls)


@pytest.mark.parametrize("world", [2, 8])
def test_cfg3_256_slot_match_sharded_over_logical_ranks(p128_keys, world):
    """BASELINE configs[2] at size: 256 slots x 8 bit, uniform bytes, `world` logical ranks of
    256/world slots each.  Every rank's decrypted partial sum equals the plaintext sum of squares
    of its slot range, their total is the distance, and the match bit is (distance > bound)
     on both sides of the threshold.  World 8 is the configuration BASELINE names (the digest test
    above pins its ciphertexts word for word but checks neither both sides of the threshold nor the plaintext partial
    sums at 8 ranks; this does)."""
    import random
    import torch
    from peba1_amd import api, circuits, lib
    from peba1_amd import dist as pd
    pp, ks, _ = p128_keys
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(2560 + world)
    rnd = random.Random(world)
    nslots = 256
    tmpl = [rnd.randrange(256) for _ in range(nslots)]
    probe = [(t + rnd.randrange(-9, 10)) % 256 or 1 for t in tmpl]
    tmpl = [t or 1 for t in tmpl]                        # a zero subtrahend trips the reference's SUBN defect
    want = [sum((a - b) ** 2 for a, b in zip(probe[lo:hi], tmpl[lo:hi]))
            for lo, hi in (pd.shard_slots(nslots, world, r) for r in range(world))]
    d = sum(want)
    assert d < (1 << 23)
    T = circuits.EncryptedVector(pp, tmpl, 8, ks).to_device()
    S = circuits.EncryptedVector(pp, probe, 8, ks).to_device()
    parts = {}
    api.reset_stats()
    api.set_deferred(True)
    try:
        outs = []
        for bound_v in (d, d - 1):
            bound = circuits.encrypt_number(pp, bound_v, 24, ks)
            res = pd.sharded_match_logical(torch, L, circuits.load(), pp.ptr, ks.cloud, pp.words,
                                           [a.ptr for a in S.slots], [a.ptr for a in T.slots], bound.ptr, 8, world,
                                           device="cuda", partial_hook=lambda r, t: parts.__setitem__(r, t.clone()))
            api.flush()
            outs.append((bound_v, C.cast(res, lib.LS)))
            if bound_v == d:
                st = api.stats()
    finally:
        api.set_deferred(False)
    # 1,683 blind rotations per slot + the adder tree + the comparator (24 XNOR, 48 MUX = 96 rotations)
    assert st["blind_rotates"] + 2 * (st["reused_gates"] + st["dead_gates"]) >= nslots * 1683 + (world - 1) * 161 + 24 + 96
    for bound_v, res in outs:
        assert L.bootsSymDecrypt(res, ks.ptr) == (1 if d > bound_v else 0), (world, bound_v)
        L.delete_gate_bootstrapping_ciphertext_array(24, res)
    tmp = api.CiphertextArray(pp, 24)
    for r in range(world):
        host = np.ascontiguousarray(parts[r].numpy())             # packed partial sums travel through host memory
        assert L.tfhe_hip_import_samples(tmp.ptr, 24, pp.ptr, host.ctypes.data_as(lib.I32P)) == 0
        assert circuits.decrypt_number(tmp, ks) == want[r], (world, r)


def test_fast_combine_gives_the_same_match_bit(p128_keys):
    """peba1_combine_and_compare_fast (carry-save compressor + prefix adder + prefix comparator on
    rank 0, ~20 levels instead of ~290 for 8 ranks): same decrypted bit as the ripple-tree combine
    and the plaintext rule, on both sides of the threshold; 8 logical ranks, one slot each."""
    import torch
    from peba1_amd import api, circuits, lib
    from peba1_amd import dist as pd
    pp, ks, _ = p128_keys
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(808)
    tmpl = [12, 200, 77, 255, 1, 90, 131, 64]
    probe = [15, 190, 78, 1, 255, 91, 140, 60]
    d = sum((a - b) ** 2 for a, b in zip(probe, tmpl))
    T = circuits.EncryptedVector(pp, tmpl, 8, ks)
    S = circuits.EncryptedVector(pp, probe, 8, ks)
    api.set_deferred(True)
    try:
        for bound_v in (d - 1, d, d + 1):
            bits, levels = [], []
            for fast in (False, True):
                bound = circuits.encrypt_number(pp, bound_v, 24, ks)
                api.reset_stats()
                res = pd.sharded_match_logical(torch, L, circuits.load(), pp.ptr, ks.cloud, pp.words,
                                               [a.ptr for a in S.slots], [a.ptr for a in T.slots], bound.ptr, 8, 8,
                                               device="cuda", fast_combine=fast)
                levels.append(api.flush())
                r = C.cast(res, lib.LS)
                bits.append(L.bootsSymDecrypt(r, ks.ptr))
                L.delete_gate_bootstrapping_ciphertext_array(24, r)
            assert bits == [1 if d > bound_v else 0] * 2, (bound_v, bits)
            assert levels[1] < 40 < levels[0], levels           # depth of rank 0's tail
    finally:
        api.set_deferred(False)


def test_cfg4_identification_streams_matches_through_bounded_flushes(p128_keys):
    """BASELINE configs[3] shape on one GPU: one probe against M independent 128-slot templates
    (full reference Function_f each), recorded `group` at a time so the slot pool bounds memory,
    every match bit equal to the plaintext rule; the genuine template is found."""
    from peba1_amd import api, circuits, identify, lib
    pp, ks, _ = p128_keys
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(1024)
    nslots, M, group = 128, 6, 3
    base = [(37 * i + 11) % 255 or 1 for i in range(nslots)]
    probe_v = [v + 1 for v in base]
    templates_v = [identify.synthetic_template(base, k + 1) for k in range(M)]      # k = 0 would be `base` itself
    genuine = 4
    templates_v[genuine] = base
    probe = circuits.EncryptedVector(pp, probe_v, 8, ks).to_device()
    templates = [circuits.EncryptedVector(pp, t, 8, ks).to_device() for t in templates_v]
    bound = circuits.encrypt_number(pp, 256, 24, ks)
    bound.set_words(bound.words())
    api.reset_stats()
    api.set_tuning("reuse_gates", 0)
    api.set_tuning("eliminate_dead", 0)
    try:
        bits_ct = identify.identify(pp, ks, probe, templates, bound, 8, group=group)
    finally:
        api.set_tuning("reuse_gates", 1)
        api.set_tuning("eliminate_dead", 1)
    st = api.stats()
    assert st["flushes"] == M // group and st["blind_rotates"] == M * 215544
    got = [int(b) for b in bits_ct.decrypt(ks)]
    want = [1 if sum((a - b) ** 2 for a, b in zip(probe_v, t)) > 256 else 0 for t in templates_v]
    assert got == want and got.count(0) == 1 and got[genuine] == 0


def test_cfg4_identification_at_the_per_gpu_size_of_configs3(p128_keys):
    """BASELINE configs[3] at its own per-GPU size (only the builder had run it): ONE probe against 128
    enrolled 128-slot x 8-bit templates -- 128 independent runs of the reference's Function_f, 27.6 M blind rotations
    -- streamed through the slot pool eight matches per flush (16 pipelined flushes, libpeba1-dist's peba1_identify), every one
    of the 128 decrypted match bits equal to the plaintext rule and the genuine template the only 0.  About four minutes on
    one MI355X."""
    import sys
    import time
    from peba1_amd import api, circuits, identify, lib
    pp, ks, _ = p128_keys
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(4096)
    nslots, M, group = 128, 128, 8
    base = [(37 * i + 11) % 255 or 1 for i in range(nslots)]
    probe_v = [v + 1 for v in base]
    templates_v = [identify.synthetic_template(base, k + 1) for k in range(M)]
    genuine = 77
    templates_v[genuine] = base
    probe = circuits.EncryptedVector(pp, probe_v, 8, ks).to_device()
    templates = [circuits.EncryptedVector(pp, t, 8, ks).to_device() for t in templates_v]
    bound = circuits.encrypt_number(pp, 256, 24, ks)
    bound.set_words(bound.words())
    api.reset_stats()
    t0 = time.time()

    def progress(first, count):          # one line per 16 matches: the run is long, show that it moves
        if (first + count) % 16 == 0:
            print(f"[identify] {first + count}/{M} matches, {time.time() - t0:.0f} s", file=sys.stderr, flush=True)

    bits_ct = identify.identify(pp, ks, probe, templates, bound, 8, group=group, on_group=progress)
    seconds = time.time() - t0
    st = api.stats()
    assert st["flushes"] == M // group
    # the library's default sharing of identical pending gates is on: executed + shared == recorded
    assert st["blind_rotates"] <= M * 215544 <= st["blind_rotates"] + 2 * (st["reused_gates"] + st["dead_gates"])
    got = [int(b) for b in bits_ct.decrypt(ks)]
    want = [1 if sum((a - b) ** 2 for a, b in zip(probe_v, t)) > 256 else 0 for t in templates_v]
    assert got == want and got.count(0) == 1 and got[genuine] == 0
    print(f"[identify] {M} matches in {seconds:.1f} s = {seconds / M * 1e3:.0f} ms per match, "
          f"{st['blind_rotates'] / seconds:.0f} executed gates/s", file=sys.stderr, flush=True)


TWO_PROCESS_WORKER = r'''
import ctypes as C, hashlib, json, os, sys
import numpy as np
import torch, torch.distributed as dist
ROOT = os.environ["PEBA1_ROOT"]
sys.path.insert(0, ROOT)
from peba1_amd import api, circuits, lib
from peba1_amd import dist as pd
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
g = json.load(open(os.path.join(ROOT, "tests", "golden", "sharded_match_digest.json")))
assert world == g["world"]
L = lib.load()
pp = api.ParameterSet(128)
ks = api.SecretKeySet(pp, g["key_seed"], device=True)            # every rank: the same keys from the same seed
L.tfhe_hip_set_encrypt_seed(g["encrypt_seed"])                     # and the same input ciphertexts (fixture order)
T, S = [], []
for t, s in zip(g["template"], g["probe"]):
    T.append(circuits.encrypt_number(pp, t, g["bits"], ks))
    S.append(circuits.encrypt_number(pp, s, g["bits"], ks))
bound = circuits.encrypt_number(pp, g["bound"], 3 * g["bits"], ks)
lo, hi = pd.shard_slots(len(T), world, rank)
seen = {}
res = pd.sharded_match(dist, torch, L, circuits.load(), pp.ptr, ks.cloud, pp.words, [a.ptr for a in S[lo:hi]],
                       [a.ptr for a in T[lo:hi]], bound.ptr, g["bits"], device="cpu",
                       partial_hook=lambda r, t: seen.__setitem__(r, hashlib.sha256(t.numpy().tobytes()).hexdigest()))
assert seen[rank] == g["partial_sha256"][rank], ("partial sums of rank", rank)
if rank == 0:
    r = C.cast(res, lib.LS)
    words = np.zeros((24, pp.words), dtype=np.int32)
    assert L.tfhe_hip_export_samples(r, 24, pp.ptr, words.ctypes.data_as(lib.I32P)) == 0
    assert hashlib.sha256(words.tobytes()).hexdigest() == g["result_b_sha256"]
    assert L.bootsSymDecrypt(r, ks.ptr) == g["match_bit"]
    print("TWO-PROCESS-OK")
dist.barrier()
dist.destroy_process_group()
'''


def _torchrun(nproc, args, port, timeout=400):
    import subprocess
    import sys
    env = dict(os.environ, PEBA1_ROOT=ROOT, MASTER_ADDR="127.0.0.1")
    return subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
                           "--master-addr", "127.0.0.1", "--master-port", str(port)] + args,
                          env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_sharded_match_in_two_processes_reproduces_the_oracle_digest(tmp_path):
    """a world >= 2 run of dist.sharded_match on the HIP path.  Two processes (gloo for the
    exchange, both on the one GPU of a test box) regenerate the same keys and inputs, each evaluates
    its slot range, ONE gather moves the partial sums, rank 0 combines: the packed partial sums of
    both ranks and the 24 outputs hash to the oracle's digests of the same DAG
    (tests/golden/sharded_match_digest.json) -- the real multi-process path, bit for bit."""
    w = tmp_path / "worker.py"
    w.write_text(TWO_PROCESS_WORKER)
    out = _torchrun(2, [str(w)], 29641)
    assert out.returncode == 0 and "TWO-PROCESS-OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def _check_rehearsal_line(out, transport="gloo", world=2):
    import json
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    j = json.loads(lines[-1])
    assert j["n_gpus"] == world and j["scaling"] == "strong" and j["config"]["mode"] == "sharded"
    assert j["value"] > 0 and j["roofline"]["frac"] > 0
    # a rank's share of 8 slots is narrow levels only: the 8-wave kernel dominates, and the binding roofline in the line is
    # THAT kernel's, measured on its launches of the timed step
    vi = j["roofline"]["valu_issue"]
    assert j["roofline"]["kernel"] == "blind_rotate8_kernel" and vi["kernel"] == "blind_rotate8_kernel<10,true>"
    assert vi["measured_cycles_per_simd_step"] > vi["chip_peak_cycles_per_simd_step"] > 0 and 0 < vi["frac_vs_chip_peak"] < vi["frac"] < 1
    # all ranks' rotations are counted: 8 slots of the reference's loop, one adder on rank 0, the comparator
    rotations = j["value"] * j["ms_per_step"] / 1e3
    assert 8 * 1683 - 1 <= rotations <= 8 * 1683 + 1000 + 200 * world, rotations
    # ... and the same line carries the weak-scaling leg: every rank's own 8 independent matches through
    # peba1_identify, the match bits gathered to rank 0 and checked there (one 0 among 16: the genuine template)
    w = j["weak_scaling"]
    assert w["n_gpus"] == world and w["matches_per_gpu"] == 8 and w["scaling"] == "weak"
    per_match = w["gates_per_s_all_ranks"] * w["seconds"] / (8 * world)
    assert 8 * 1683 <= per_match <= 8 * 1683 + 400, per_match
    # the same match once more with SURVEY 8(e)'s combine on rank 0 (ripple-adder tree + bit-serial comparator)
    r = j["reference_order_combine"]
    assert r["match_ms"] > 0 and 8 * 1683 <= r["blind_rotates_all_ranks"] <= 8 * 1683 + 1000 + 500 * world
    # who took part: two ranks, each naming the device libtfhe-hip ran on; on the one GPU of a test box
    # both name the same bus id and the line says so
    d = j["dist"]
    assert d["world"] == world and len(d["devices"]) == world and all(d["devices"]) and d["library_transport"] == "host" and transport in d["transport"]
    assert d["distinct_devices"] == 1 and d["one_gpu_per_rank"] is False
    # exactly the collectives the run is made of (--steps 1 --warmup 0): the timed step's gather of the partial sums, the
    # weak leg's broadcast of the probe and gather of the match bits, the reference-order leg's gather; over the host
    # transport a status word rides in front of every payload
    assert d["data_collectives"] == {"gathers": 3, "broadcasts": 1} and d["status_word_collectives"] == 4
    # ... issued in the same order on every rank (peba1_dist_sequence: count + rolling hash of kind / size / root)
    assert d["collectives_issued_rank0"] == 4 and d["same_issue_order_on_every_rank"] is True
    assert len({e["collectives"]["issue_order_hash"] for e in d["ranks"]}) == 1
    assert [e["rank"] for e in d["ranks"]] == list(range(world)) and len({e["pid"] for e in d["ranks"]}) == world
    return j


def test_bench_fallback_transport_moves_the_same_ciphertexts():
    """The transport bench.py falls back to when libpeba1-dist's own RCCL communicator cannot be made on a node (first
    contact with several GPUs happens in the driver's run, not here): the library's host transport carried by the torch
    group's collectives on DEVICE tensors.  Rehearsed over gloo (two ranks cannot share one GPU under RCCL); the same checks
    as the default rehearsal -- match bit, rotation counts, gathered match bits, both combines."""
    out = _torchrun(2, ["bench.py", "--gpus", "2", "--backend", "gloo", "--transport", "torch", "--steps", "1", "--warmup", "0", "--full",
                        "--slots", "8", "--no-cpu-baseline"], 29645)
    j = _check_rehearsal_line(out, transport="torch.distributed device tensors")
    assert j["dist"]["transport_fallback_reason"] == "--transport torch"


def test_bench_launches_its_own_ranks_when_called_without_a_launcher():
    """`python bench.py --gpus 4` with no WORLD_SIZE in the environment -- how the driver
    calls it at N = 1 -- must produce the N = 4 line by itself: the parent starts one fresh process per rank (it never
    touches the GPU), relays rank 0's JSON line as its own last stdout line and exits 0.  What the ranks then run is what
    the driver's `torch.distributed.run ... bench.py --gpus N` runs at N > 1 -- mode auto = sharded: slots partitioned over
    the ranks, one gather, rank 0 combines, barrier + max-over-ranks timing, one JSON line from rank 0 -- rehearsed with
    FOUR processes on one GPU (--backend gloo), 8 slots: world 4, the exact collective counts, the same issue order on
    every rank.  A rehearsal of the code path, not a measurement."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PEBA1_ROOT"] = ROOT
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--backend", "gloo", "--steps", "1", "--warmup", "0", "--full",
                          "--slots", "8", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    j = _check_rehearsal_line(out, world=4)
    assert out.stdout.rstrip().splitlines()[-1].startswith("{")           # the line is the LAST thing on stdout
    assert j["dist"]["torch_backend"] == "gloo"


@pytest.mark.parametrize("hang", [False, True])
def test_bench_tries_its_own_communicator_in_a_child_process_first(hang):
    """before a rank makes libpeba1-dist's own RCCL communicator, the same communicator and one one-sample gather
    are tried in a child process per rank; only if every rank's child reports success does the rank itself enter
    ncclCommInitRank.  World 1 over RCCL on the one GPU (`--force-dist`).  hang = False: the child succeeds, the library's
    own communicator carries the exchange and its status words travel on a communicator of their own (ncclCommSplit).
    hang = True: the child never comes back (test hook), is killed at its budget, and the run still produces its line over
    the fallback transport, saying why."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MASTER_PORT="29671", PEBA1_BENCH_TRIAL_BUDGET_S="12" if hang else "150")
    if hang:
        env["PEBA1_BENCH_TRIAL_HANG"] = "1"
    out = subprocess.run([sys.executable, "bench.py", "--mode", "sharded", "--force-dist", "--steps", "1", "--warmup", "0", "--full", "--slots", "8",
                          "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    d = j["dist"]
    assert d["world"] == 1 and d["backend"] == "rccl" and d["rccl_version"] > 0 and d["same_issue_order_on_every_rank"] is True
    if hang:
        assert "torch.distributed device tensors" in d["transport"] and d["library_transport"] == "host"
        assert "did not finish within 12 s" in d["transport_fallback_reason"]
        assert "falling back to torch's" in out.stderr
    else:
        assert d["transport"].startswith("rccl: libpeba1-dist's own communicator") and d["library_transport"] == "rccl"
        assert d["transport_fallback_reason"] is None
        assert d["status_channel"] == "own communicator (ncclCommSplit), own stream"
        assert d["data_collectives"] == {"gathers": 3, "broadcasts": 1} and d["status_word_collectives"] == 4
