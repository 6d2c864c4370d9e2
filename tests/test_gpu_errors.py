"""GPU tests of the robustness items of VERDICT r1 / ADVICE r1: recoverable conditions are
reported through tfhe_hip_last_error() instead of aborting the host; a deferred bootsNOT is
flushed by the next decrypt; import/export follow the parameter set they are given."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    from peba1_amd import lib
    return lib.load().tfhe_hip_last_error().decode()


def test_deferred_not_is_flushed_by_decrypt(p128_keys, oracle):
    """ADVICE r1 (shim.cpp:170): bootsNOT of an already materialised ciphertext is pending at
    level 0; a bootsSymDecrypt / immediate bootsCOPY right after it -- no explicit flush -- must
    run it first, not read an unwritten slot."""
    from peba1_amd import api, lib
    pp, ks, oks = p128_keys
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(61)
    for bit in (0, 1):
        x = api.CiphertextArray(pp, 1).encrypt([bit], ks)
        w = x.words()
        r = api.CiphertextArray(pp, 2)
        api.set_deferred(True)
        try:
            L.bootsNOT(r.at(0), x.at(0), ks.cloud)
            assert L.bootsSymDecrypt(r.at(0), ks.ptr) == 1 - bit          # no flush in between
            L.bootsNOT(r.at(1), x.at(0), ks.cloud)
        finally:
            api.set_deferred(False)                                        # leaves deferred mode: flushes
        assert (r.words()[0] == oks.gate_not(w[0])).all()
        assert (r.words()[1] == oks.gate_not(w[0])).all()
    # NOT of a fresh (never written) sample, deferred, then an immediate-mode COPY of the result
    z = api.CiphertextArray(pp, 1)
    r = api.CiphertextArray(pp, 2)
    api.set_deferred(True)
    L.bootsNOT(r.at(0), z.at(0), ks.cloud)
    api.set_deferred(False)
    L.bootsCOPY(r.at(1), r.at(0), ks.cloud)
    assert list(r.decrypt(ks)) == [1, 1]
    assert (r.words()[1] == oks.gate_not(oks.constant(0))).all()


def test_import_export_alternate_parameter_sets(p128_keys, oracle):
    """ADVICE r1 (shim.cpp:696): words imported for one parameter set right after gates of another
    ran must land in their own pool (right stride), and a device import must work before any gate
    of that set has run."""
    import torch
    from peba1_amd import api, lib
    pp, ks, oks = p128_keys
    L = lib.load()
    p80 = api.ParameterSet(80)
    k80 = api.SecretKeySet(p80, 0x80AA, device=True)
    o80 = oracle.KeySet(oracle.params("P80"), 0x80AA)
    try:
        L.tfhe_hip_set_encrypt_seed(62)
        a128 = api.CiphertextArray(pp, 2).encrypt([1, 1], ks)
        a80 = api.CiphertextArray(p80, 2).encrypt([1, 0], k80)
        w128, w80 = a128.words(), a80.words()
        # device import of P80 words before any P80 gate (and after P128 gates of the session)
        t = torch.from_numpy(w80.copy()).cuda()
        d80 = api.CiphertextArray(p80, 2)
        assert L.tfhe_hip_import_samples_device(d80.ptr, 2, p80.ptr, t.data_ptr()) == 0, _err()
        r80 = api.CiphertextArray(p80, 1)
        L.bootsAND(r80.at(0), d80.at(0), d80.at(1), k80.cloud)           # last key used: P80
        # now P128 words: must bind to the P128 pool although the last gate was P80
        b128 = api.CiphertextArray(pp, 2).set_words(w128)
        r128 = api.CiphertextArray(pp, 1)
        L.bootsAND(r128.at(0), b128.at(0), b128.at(1), ks.cloud)
        c80 = api.CiphertextArray(p80, 2).set_words(w80)                  # and back
        x80 = api.CiphertextArray(p80, 1)
        L.bootsXOR(x80.at(0), c80.at(0), c80.at(1), k80.cloud)
        assert (r80.words()[0] == o80.gate("AND", w80[0], w80[1])).all()
        assert (r128.words()[0] == oks.gate("AND", w128[0], w128[1])).all()
        assert (x80.words()[0] == o80.gate("XOR", w80[0], w80[1])).all()
        out = torch.zeros(2 * pp.words, dtype=torch.int32, device="cuda")
        assert L.tfhe_hip_export_samples_device(b128.ptr, 2, pp.ptr, out.data_ptr()) == 0, _err()
        assert (out.cpu().numpy().reshape(2, -1) == w128).all()
        # a P128 array handed over with P80 parameters is refused, not mis-strided
        L.tfhe_hip_clear_error()
        bad = np.zeros(2 * p80.words, dtype=np.int32)
        assert L.tfhe_hip_export_samples(b128.ptr, 2, p80.ptr, bad.ctypes.data_as(lib.I32P)) == -1
        assert "LWE dimension" in _err()
    finally:
        k80.close()


def test_sample_used_with_a_key_of_another_dimension_is_refused(p128_keys):
    """VERDICT r1 item 7 (shim.cpp:68): reported, result untouched, process alive."""
    from peba1_amd import api, lib
    pp, ks, _ = p128_keys
    L = lib.load()
    p80 = api.ParameterSet(80)
    k80 = api.SecretKeySet(p80, 0x80AB, device=True)
    try:
        L.tfhe_hip_set_encrypt_seed(63)
        a = api.CiphertextArray(pp, 2).encrypt([1, 1], ks)
        r = api.CiphertextArray(pp, 1)
        L.bootsAND(r.at(0), a.at(0), a.at(1), ks.cloud)                   # binds the arrays to P128
        before = r.words().copy()
        L.tfhe_hip_clear_error()
        L.bootsXOR(r.at(0), a.at(0), a.at(1), k80.cloud)                   # wrong key
        assert "different LWE dimension" in _err()
        assert (r.words() == before).all() and r.decrypt(ks)[0] == 1
        L.tfhe_hip_clear_error()
        L.bootsMUX(r.at(0), a.at(0), a.at(1), a.at(1), k80.cloud)
        assert "different LWE dimension" in _err() and (r.words() == before).all()
        L.tfhe_hip_clear_error()
        L.bootsNOT(r.at(0), a.at(0), k80.cloud)
        assert "different LWE dimension" in _err() and (r.words() == before).all()
        # still usable afterwards
        L.tfhe_hip_clear_error()
        L.bootsXOR(r.at(0), a.at(0), a.at(1), ks.cloud)
        assert _err() == "" and r.decrypt(ks)[0] == 0
    finally:
        k80.close()


POOL_WORKER = r'''
import sys
sys.path.insert(0, %r)
from peba1_amd import api, lib
L = lib.load()
pp = api.ParameterSet(128)
ks = api.SecretKeySet(pp, 7, device=True)
L.tfhe_hip_set_encrypt_seed(5)
w = api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
L.bootsAND(w.at(2), w.at(0), w.at(1), ks.cloud)            # first gate: the slot pool exists from here on
assert w.decrypt(ks)[2] == 1
w.close()
held = []
# 64-slot pool: hold ciphertext arrays until no slot is left (materialised inputs pin one each)
refused = None
for i in range(200):
    a = api.CiphertextArray(pp, 1).encrypt([1], ks)
    L.tfhe_hip_clear_error()
    rc = L.tfhe_hip_import_samples(a.ptr, 1, pp.ptr, a.words().ctypes.data_as(lib.I32P))
    if rc != 0:
        refused = (i, L.tfhe_hip_last_error().decode())
        break
    held.append(a)
assert refused is not None and "slot pool exhausted" in refused[1], refused
assert 40 < refused[0] <= 64, refused
# a gate while the pool is dry: refused, reported, the result keeps its old value
r = api.CiphertextArray(pp, 1).encrypt([0], ks)
L.tfhe_hip_clear_error()
L.bootsAND(r.at(0), held[0].at(0), held[1].at(0), ks.cloud)
assert "slot pool exhausted" in L.tfhe_hip_last_error().decode()
assert r.decrypt(ks)[0] == 0
# free some arrays: the same call now works
for a in held[:8]:
    a.close()
L.tfhe_hip_clear_error()
L.bootsAND(r.at(0), held[8].at(0), held[9].at(0), ks.cloud)
assert L.tfhe_hip_last_error().decode() == "" and r.decrypt(ks)[0] == 1
print("POOL-OK", refused[0])
'''


def test_pool_exhaustion_is_reported_not_fatal():
    """VERDICT r1 item 7 (engine.cpp:50): a dry slot pool refuses the call and says so; the
    process goes on and the call succeeds once arrays are freed."""
    env = dict(os.environ, TFHE_HIP_POOL_SLOTS="64")
    out = subprocess.run([sys.executable, "-c", POOL_WORKER % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "POOL-OK" in out.stdout


OOM_WORKER = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from peba1_amd import api, lib
L = lib.load()
pp = api.ParameterSet(128)
# (0) the device image of a key (118 MiB at P128): with no room for it the keyset is not made, the reason is reported, and the
# same call works once there is room
L.tfhe_hip_test_set_alloc_cap(1 << 20)
try:
    api.SecretKeySet(pp, 7, device=True)
    raise SystemExit("a key image was uploaded past the cap")
except RuntimeError as e:
    assert "out of device memory" in str(e) and "key" in str(e), str(e)
L.tfhe_hip_test_set_alloc_cap(0)
ks = api.SecretKeySet(pp, 7, device=True)
L.tfhe_hip_set_encrypt_seed(5)
G = 5000
rng = np.random.default_rng(1)
xa, xb = rng.integers(0, 2, G), rng.integers(0, 2, G)
a = api.CiphertextArray(pp, G).encrypt(xa, ks)
b = api.CiphertextArray(pp, G).encrypt(xb, ks)
r = api.CiphertextArray(pp, G)
api.set_deferred(True)
for i in range(4):                                             # a first, small flush: pool and small scratch exist
    L.bootsAND(r.at(i), a.at(i), b.at(i), ks.cloud)
assert api.flush() >= 0
# (1) the scratch of a flush: a 5,000-wide level needs ~0.6 GB of key-switch partial sums; with 64 MiB of headroom the
# flush is refused, says why, and the gates stay recorded
L.tfhe_hip_test_set_alloc_cap(64 << 20)                        # less than what is already held: nothing more may be allocated
for i in range(G):
    L.bootsAND(r.at(i), a.at(i), b.at(i), ks.cloud)
L.tfhe_hip_clear_error()
assert api.flush() == -1
msg = L.tfhe_hip_last_error().decode()
assert "out of device memory" in msg and "scratch" in msg, msg
assert api.flush() == -1                                       # still pending, still refused
L.tfhe_hip_test_set_alloc_cap(0)
L.tfhe_hip_clear_error()
assert api.flush() >= 1 and L.tfhe_hip_last_error().decode() == ""
assert (r.decrypt(ks) == (xa & xb)).all()
# (1b) a refused flush with dead gates pending: elimination has released their result slots, which the next gates of the
# retry get again (the pool's free list is LIFO).  Recording the same gates again must not share those freed slots, and a
# NOT of a gate that got a dead NOT's slot must not be aliased to that NOT's operand.  A multi-output op (AND and NAND
# of a[j], b[j] from one rotation of t = a + b + 1/8) loses its dead output at the refused flush and is widened by it again.
K = 8
and_nand = api.LutMulti.from_tables(pp, 1 << 29, [[-1, 1], [1, -1]])
mand, mnand = api.CiphertextArray(pp, K), api.CiphertextArray(pp, K)
w = api.CiphertextArray(pp, G)                                 # with r: a level twice as wide as (1)'s, so its scratch must grow
dead2, deadmux, deadnot, notnot = (api.CiphertextArray(pp, K) for _ in range(4))
for i in range(G):
    L.bootsXOR(r.at(i), a.at(i), b.at(i), ks.cloud)
    L.bootsOR(w.at(i), a.at(i), b.at(i), ks.cloud)
def record_dying():
    for j in range(K):
        L.bootsNAND(dead2.at(j), a.at(j), b.at(j), ks.cloud)
        L.bootsMUX(deadmux.at(j), a.at(j), b.at(j), b.at(j + 1), ks.cloud)
        L.bootsNOT(deadnot.at(j), a.at(j), ks.cloud)
        L.bootsNOT(notnot.at(j), deadnot.at(j), ks.cloud)         # NOT of a pending NOT: aliases a[j]
        api.lut_bootstrap_multi(and_nand, [mand.at(j), mnand.at(j)], [a.at(j), b.at(j)], [1, 1], 1 << 29, ks)
record_dying()
for arr in (dead2, deadmux, deadnot, mnand):                        # overwritten before the flush: the gates above are dead
    for j in range(K):
        L.bootsCONSTANT(arr.at(j), 0, ks.cloud)
L.tfhe_hip_test_set_alloc_cap(64 << 20)
assert api.flush() == -1
record_dying()                                                 # the same gates again
fresh, freshnot = api.CiphertextArray(pp, 3 * K), api.CiphertextArray(pp, 3 * K)
for j in range(3 * K):                                         # as many new, distinct gates as died
    L.bootsANDYN(fresh.at(j), a.at(K + j), b.at(2 * K + j), ks.cloud)
    L.bootsNOT(freshnot.at(j), fresh.at(j), ks.cloud)
L.tfhe_hip_test_set_alloc_cap(0)
L.tfhe_hip_clear_error()
assert api.flush() >= 1 and L.tfhe_hip_last_error().decode() == ""
xs, xs1 = xa[:K], xb[1:K + 1]
assert (r.decrypt(ks) == (xa ^ xb)).all() and (w.decrypt(ks) == (xa | xb)).all()
assert (dead2.decrypt(ks) == 1 - (xa[:K] & xb[:K])).all()
assert (deadmux.decrypt(ks) == np.where(xs == 1, xb[:K], xs1)).all()
assert (deadnot.decrypt(ks) == 1 - xs).all() and (notnot.decrypt(ks) == xs).all()
assert (mand.decrypt(ks) == (xa[:K] & xb[:K])).all() and (mnand.decrypt(ks) == 1 - (xa[:K] & xb[:K])).all()
want_fresh = xa[K:4 * K] & (1 - xb[2 * K:5 * K])
assert (fresh.decrypt(ks) == want_fresh).all() and (freshnot.decrypt(ks) == 1 - want_fresh).all()
for arr in (w, dead2, deadmux, deadnot, notnot, fresh, freshnot, mand, mnand, and_nand):
    arr.close()
# (2) the slot pool's growth (it starts at 65,536 slots): the gate that needs slot 65,537 is refused and has no effect;
# with the cap lifted the same call works and every gate recorded before it still evaluates
L.tfhe_hip_test_set_alloc_cap(1 << 20)
big = api.CiphertextArray(pp, 70000)
refused = None
for i in range(70000):
    L.tfhe_hip_clear_error()
    L.bootsXOR(big.at(i), a.at(i %% G), b.at((i + i // G) %% G), ks.cloud)       # a pair of operands never repeats: no gate is shared
    e = L.tfhe_hip_last_error().decode()
    if e:
        refused = (i, e)
        break
assert refused is not None and "out of device memory" in refused[1] and "slot pool" in refused[1], refused
assert 40000 < refused[0] < 65536, refused
L.tfhe_hip_test_set_alloc_cap(0)
L.tfhe_hip_clear_error()
for i in range(refused[0], refused[0] + 2000):
    L.bootsXOR(big.at(i), a.at(i %% G), b.at((i + i // G) %% G), ks.cloud)
assert L.tfhe_hip_last_error().decode() == ""
n = refused[0] + 2000
got = big.decrypt(ks)[:n]
want = np.array([xa[i %% G] ^ xb[(i + i // G) %% G] for i in range(n)])
assert (got == want).all()
print("OOM-OK", refused[0])
'''


def test_device_memory_exhaustion_is_recoverable():
    """hipErrorOutOfMemory while uploading a key image, sizing a flush's scratch or growing the slot pool
    (here: an artificial cap, tfhe_hip_test_set_alloc_cap) does not abort the host: the keyset is not made / the flush returns -1 / the gate call has no effect,
    tfhe_hip_last_error() names what could not be allocated, the recorded gates stay recorded and evaluate once memory
    is there."""
    out = subprocess.run([sys.executable, "-c", OOM_WORKER % ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "OOM-OK" in out.stdout


def test_pool_size_is_bounded_by_the_gate_key_fields():
    """TFHE_HIP_POOL_SLOTS beyond what the pending-gate keys can hold (2^29) is
    clamped and reported instead of letting two gates share a key."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from peba1_amd import api, lib\n"
            "L = lib.load(); pp = api.ParameterSet(128)\n"
            "ks = api.SecretKeySet(pp, 7, device=True)\n"
            "a = api.CiphertextArray(pp, 2).encrypt([1, 1], ks); r = api.CiphertextArray(pp, 1)\n"
            "L.bootsAND(r.at(0), a.at(0), a.at(1), ks.cloud)\n"
            "print('ERR', L.tfhe_hip_last_error().decode()); print('BIT', r.decrypt(ks)[0])\n" % ROOT)
    env = dict(os.environ, TFHE_HIP_POOL_SLOTS="4")          # below the minimum: clamped up to 8
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "TFHE_HIP_POOL_SLOTS out of range" in out.stdout and "BIT 1" in out.stdout


def test_gadget_outside_every_kernel_form_is_refused_at_key_upload():
    """N = 2048, l = 8, Bgbit = 4 passes the CRT range check but exceeds the lazy-arithmetic bounds of every
    blind-rotate form (br_forms.hpp): the keyset is refused with a message instead of evaluating wrong ciphertexts."""
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(custom=(8, 2048, 1, 8, 4, 8, 2, 2.0 ** -15, 2.0 ** -25, 0.012467))
    L.tfhe_hip_clear_error()
    with pytest.raises(RuntimeError, match="every blind-rotate kernel form"):
        api.SecretKeySet(pp, 7, device=True)


def test_device_identity_and_bounded_event_wait(p128_keys):
    """Round 5 entry points: the PCI bus id of the device the library runs on (what bench.py prints per rank as evidence of N
    distinct GPUs) and the bounded wait on a caller's own HIP event (what libpeba1-dist reads the status words of a
    collective back with).  The library binds the calling thread to its device only for the duration of a call: the
    caller's current device is the same before and after."""
    import ctypes as C
    import re
    import torch
    from peba1_amd import api, lib
    pp, ks, _ = p128_keys
    L = lib.load()
    before = torch.cuda.current_device()
    buf = C.create_string_buffer(64)
    assert L.tfhe_hip_device_pci_bus_id(buf, 64) == 0
    assert re.fullmatch(r"[0-9a-fA-F]{4}:[0-9a-fA-F]{2}:[0-9a-fA-F]{2}\.[0-9a-fA-F]", buf.value.decode()), buf.value
    assert L.tfhe_hip_device_pci_bus_id(buf, 4) == -1 and "16 bytes" in _err()
    # an event of the caller's own, recorded behind work on the library's stream
    a = api.CiphertextArray(pp, 64).encrypt([1] * 64, ks)
    r = api.CiphertextArray(pp, 64)
    api.set_deferred(True)
    try:
        for i in range(64):
            L.bootsAND(r.at(i), a.at(i), a.at(i), ks.cloud)
        api.flush_async()                                         # enqueued, not waited for
        stream = torch.cuda.ExternalStream(L.tfhe_hip_stream())
        ev = torch.cuda.Event()
        ev.record(stream)
        assert L.tfhe_hip_wait_event(C.c_void_p(ev.cuda_event), b"test event") == 0
        assert ev.query()                                         # the wait returned because the event had completed
        assert L.tfhe_hip_wait_event(None, b"null") == -1
    finally:
        api.set_deferred(False)
    assert list(r.decrypt(ks)) == [1] * 64
    assert torch.cuda.current_device() == before
