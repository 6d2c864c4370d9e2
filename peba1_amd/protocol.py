"""Protocol P_1 as the reference's driver runs it (src/main.cpp:533-586): the client's
encrypted sample is matched against the stored encrypted template with Function_f, the
server draws two random bytes r0, r1, Function_g turns the encrypted match bit into an
encryption of one of them, the client decrypts it and is authenticated when it returns r1.

The driver reproduces the reference's behaviour, not its intent: Function_f's bit is 1 when
the distance EXCEEDS the bound and Function_g returns r1 for bit 1, so the reference
"authenticates" exactly the samples that do not match, and for bit 0 its
|1 - 0| = 255 (bootsSUBNbit, Math.cpp:137-138) makes y = 255*r0 mod 256 rather than r0.
`function_f=circuits.function_f_fast` swaps in the optimised DAG (same match bit).

Host plumbing only; every gate goes through the boots* C ABI of libtfhe-hip.so.  Each
function runs in deferred mode and is flushed by the decryption (or the explicit flush)
that follows it.

    python -m peba1_amd.protocol --nslots 128            # genuine and impostor run, one GPU
    python -m peba1_amd.protocol --clients 4             # four clients, each with a key pair of its own, batched
    python -m peba1_amd.protocol --compressed-keys       # the cloud key travels as a seed and the bodies (10x fewer bytes)
    python -m peba1_amd.protocol --seeded-inputs         # template and sample travel as seed-compressed ring samples
    python -m peba1_amd.protocol --seeded-lwe            # template and sample travel as seed-compressed LWE sample arrays
    python -m peba1_amd.protocol --ring-lut              # an encrypted 8-entry table under an index the server computed
    python -m peba1_amd.protocol --packed-gallery        # Hamming match of one claimed identity against a packed gallery
    python -m peba1_amd.protocol --seeded-selectors      # select, packed lookup and inner products, the TGSW material seed-compressed

With --clients K the server side runs as a multi-user server does: Function_f of all K clients in ONE flush and
Function_g of all K in a second one (multi-key flushes, tuning "batch_keys"), one JSON line per client.
"""
import argparse
import json
import time

import numpy as np

from . import api, circuits

MAX_BITSIZE = 24        # 3 * bitsize: width of the distance and of result_b (main.cpp:46)


def shipped_vector(params, values, bitsize, key, ev):
    """What --seeded-inputs puts between client and server: the client encrypts the features as ONE seed-compressed ring
    sample (10 + N words: a fresh mask seed and the body), the server opens it on the device under its cloud key."""
    words = circuits.ring_encrypt_vector(values, bitsize, key, compressed=True)
    return circuits.EncryptedVector.from_ring(params, words, len(values), bitsize, ev)


def shipped_lwe_vector(params, values, bitsize, key):
    """What --seeded-lwe puts between client and server: the client encrypts the features as ONE seed-compressed record of
    fresh LWE samples (10 + nslots * bitsize words: a fresh mask seed and one body per bit), the server opens it on the
    device -- no cloud key is involved and no key switch is paid."""
    words = circuits.seeded_lwe_encrypt_vector(values, bitsize, key)
    return circuits.EncryptedVector.from_seeded_lwe(params, words, len(values), bitsize)


def run_p1(params, key, sample, template, bound_match, r0, r1, bitsize=8, cloud=None, function_f=None, seeded_inputs=False,
           seeded_lwe=False):
    """One protocol run.  `key` is the client's secret keyset (encrypts, decrypts); `cloud`
    (default: its embedded cloud keyset) is all the evaluating side uses.  Returns a dict with
    the decrypted y, whether the client was authenticated (y == r1, main.cpp:578) and timings.
    seeded_inputs: template and sample travel as seed-compressed ring samples (shipped_vector); seeded_lwe: as one
    seed-compressed LWE record per vector (shipped_lwe_vector)."""
    ev = key if cloud is None else cloud
    t0 = time.perf_counter()
    if seeded_lwe:
        enc_template = shipped_lwe_vector(params, template, bitsize, key)
        enc_sample = shipped_lwe_vector(params, sample, bitsize, key)
    elif seeded_inputs:
        enc_template = shipped_vector(params, template, bitsize, key, ev)
        enc_sample = shipped_vector(params, sample, bitsize, key, ev)
    else:
        enc_template = circuits.EncryptedVector(params, template, bitsize, key).to_device()
        enc_sample = circuits.EncryptedVector(params, sample, bitsize, key).to_device()
    enc_bound = circuits.encrypt_number(params, bound_match, MAX_BITSIZE, key)
    enc_r0 = circuits.encrypt_number(params, r0, bitsize, key)           # main.cpp:553-559
    enc_r1 = circuits.encrypt_number(params, r1, bitsize, key)
    t_enc = time.perf_counter()
    was_deferred = api.get_deferred()
    api.set_deferred(True)
    try:
        enc_b = api.CiphertextArray(params, MAX_BITSIZE)
        (function_f or circuits.function_f)(enc_b, enc_sample, enc_template, enc_bound, bitsize, ev)    # main.cpp:538
        levels_f = api.flush()
        t_f = time.perf_counter()
        enc_y = api.CiphertextArray(params, bitsize + 1)
        circuits.function_g(enc_y, enc_b, enc_r0, enc_r1, bitsize, ev)                 # main.cpp:564
        levels_g = api.flush()
        t_g = time.perf_counter()
    finally:
        api.set_deferred(was_deferred)
    y = circuits.decrypt_number(enc_y, key, bitsize)                                   # main.cpp:571-575
    b = int(enc_b.decrypt(key)[0])
    return {"y": y, "r0": r0, "r1": r1, "match_bit": b, "authenticated": y == r1,
            "seconds": {"encrypt": t_enc - t0, "function_f": t_f - t_enc, "function_g": t_g - t_f},
            "levels": {"function_f": levels_f, "function_g": levels_g}}


def run_p1_clients(params, keys, samples, templates, bounds, r0s, r1s, bitsize=8, fast=False, clouds=None):
    """run_p1 for K clients at once, client c with its own secret keyset keys[c]: every client's Function_f in one flush,
    every Function_g in a second.  clouds[c] (default: the cloud keyset embedded in keys[c]) is all the evaluating side
    uses.  Returns one dict per client, as run_p1's (the timings are the batch's)."""
    from . import lib
    k = len(keys)
    ev = keys if clouds is None else clouds
    t0 = time.perf_counter()
    enc_t = [circuits.EncryptedVector(params, templates[c], bitsize, keys[c]).to_device() for c in range(k)]
    enc_s = [circuits.EncryptedVector(params, samples[c], bitsize, keys[c]).to_device() for c in range(k)]
    enc_bound = [circuits.encrypt_number(params, bounds[c], MAX_BITSIZE, keys[c]) for c in range(k)]
    enc_r0 = [circuits.encrypt_number(params, r0s[c], bitsize, keys[c]) for c in range(k)]
    enc_r1 = [circuits.encrypt_number(params, r1s[c], bitsize, keys[c]) for c in range(k)]
    t_enc = time.perf_counter()
    enc_b = [api.CiphertextArray(params, MAX_BITSIZE) for _ in range(k)]
    levels_f = circuits.function_f_batch(enc_b, enc_s, enc_t, enc_bound, bitsize, ev, fast=fast)
    t_f = time.perf_counter()
    enc_y = [api.CiphertextArray(params, bitsize + 1) for _ in range(k)]
    L = lib.load()
    was_deferred, had_batch = api.get_deferred(), L.tfhe_hip_set_batch_keys(1)
    api.set_deferred(True)
    try:
        for c in range(k):
            circuits.function_g(enc_y[c], enc_b[c], enc_r0[c], enc_r1[c], bitsize, ev[c])
        levels_g = api.flush()
    finally:
        api.set_deferred(was_deferred)
        L.tfhe_hip_set_batch_keys(had_batch)
    t_g = time.perf_counter()
    out = []
    for c in range(k):
        y = circuits.decrypt_number(enc_y[c], keys[c], bitsize)
        b = int(enc_b[c].decrypt(keys[c])[0])
        out.append({"client": c, "y": y, "r0": r0s[c], "r1": r1s[c], "match_bit": b, "authenticated": y == r1s[c],
                    "seconds": {"encrypt": t_enc - t0, "function_f": t_f - t_enc, "function_g": t_g - t_f},
                    "levels": {"function_f": levels_f, "function_g": levels_g}})
    return out


def client_inputs(c, nslots, seed):
    """Inputs of client c of a --clients run: its own key seed, template, sample (genuine for even c, impostor for odd
    c) and server randomness."""
    template = [(37 * i + 11 + 5 * c) % 255 for i in range(nslots)]
    sample = [t + 1 for t in template] if c % 2 == 0 else [(91 * i + 5 + 3 * c) % 256 for i in range(nslots)]
    return {"key_seed": seed + 1 + c, "template": template, "sample": sample, "r0": (17 + c) % 256, "r1": (99 + 7 * c) % 256}


def shipped_selector(params, key, bits=None, polys=None, seeded=False):
    """What travels for a selector or a TGSW probe, and the server's object made from it: the plain words, or with `seeded`
    ONE seed-compressed record (ten seed words and the bodies, half the bytes; the masks are written on the card at first
    use).  Returns (selector, bytes sent, bytes the plain words would have been)."""
    count = len(bits) if polys is None else len(polys)
    plain_bytes = 4 * count * api.tgsw_words(params)
    if seeded:
        record = (api.tgsw_encrypt_bits_compressed(bits, key) if polys is None else api.tgsw_encrypt_polys_compressed(polys, key))
        return api.Selector.from_compressed(params, record), int(record.nbytes), plain_bytes
    words = api.tgsw_encrypt_bits(bits, key) if polys is None else api.tgsw_encrypt_polys(polys, key)
    return api.Selector(params, words), int(words.nbytes), plain_bytes


def run_private_select(params, key, templates, claimed, bitsize=8, seeded_selectors=False):
    """Verification against a claimed identity by the CMUX tree alone: the gallery rests as one ring sample per template
    (circuits.ring_encrypt_vector), the client sends the TGSW-encrypted bits of `claimed`, the server selects
    (identify.select_template) and the client decrypts the selected template.  Returns one dict."""
    from . import identify
    M = len(templates)
    d = max((M - 1).bit_length(), 1)
    gallery = np.stack([circuits.ring_encrypt_vector(t, bitsize, key) for t in templates])  # enrolment, on the client
    selector, sent, plain = shipped_selector(params, key, bits=[(claimed >> j) & 1 for j in range(d)], seeded=seeded_selectors)
    t0 = time.perf_counter()
    got = identify.select_template(selector, gallery, params, len(templates[claimed]), bitsize, key)
    t_select = time.perf_counter()
    values = [circuits.decrypt_number(s, key) for s in got.slots]
    out = {"run": "select", "entries": M, "selector_bits": d, "selected_is_claimed": values == list(templates[claimed]),
           "selector_bytes": sent, "selector_bytes_plain": plain, "selector_upload_bytes": selector.upload_bytes(),
           "seconds": {"select_and_unpack": t_select - t0}}
    selector.close()
    return out


def run_packed_gallery(params, key, templates, claimed, probes, bound, width=128, cloud=None, seeded_selectors=False):
    """Verification of a claimed identity the server must not learn, against a gallery of `width`-bit templates that rests
    packed (identify.pack_gallery: N / width templates per ring sample).  The client sends the TGSW-encrypted bits of
    `claimed` and, per run, an encrypted probe; the server looks the template up (identify.lookup_template: the CMUX tree
    over the samples, one rotation step per low index bit, the unpack of `width` coefficients) and runs
    peba1_hamming_match on it.  probes: {name: bits}.  Returns one dict per probe: the decrypted bit (1 = the distance
    exceeds `bound`, the polarity of Function_f), the plaintext distance and the timings."""
    from . import identify
    ev = key if cloud is None else cloud
    M = len(templates)
    d = max((params.N // width).bit_length() - 1 + max(api.lookup_samples(params, M, width) - 1, 0).bit_length(), 1)
    t0 = time.perf_counter()
    gallery = identify.pack_gallery(templates, width, key)                               # enrolment, on the client
    selector, sent, plain = shipped_selector(params, key, bits=[(claimed >> j) & 1 for j in range(d)], seeded=seeded_selectors)
    cw = circuits.hamming_count_bits(width)
    enc_bound = circuits.encrypt_number(params, bound, cw, key)
    t_enc = time.perf_counter()
    out = []
    was_deferred = api.get_deferred()
    api.set_deferred(True)
    try:
        for name, bits in probes.items():
            t1 = time.perf_counter()
            probe = api.CiphertextArray(params, width).encrypt(bits, key)
            template = identify.lookup_template(selector, gallery, M, width, ev)
            t_lookup = time.perf_counter()
            enc_b = api.CiphertextArray(params, cw)
            circuits.hamming_match(enc_b, probe, template, width, enc_bound, ev)
            levels = api.flush()
            t_match = time.perf_counter()
            distance = sum(int(a) ^ int(b) for a, b in zip(bits, templates[claimed]))
            out.append({"run": name, "match_bit": int(enc_b.decrypt(key)[0]), "distance": distance, "bound": bound,
                        "expected_bit": int(distance > bound), "entries": M, "width": width, "selector_bits": d,
                        "gallery_bytes": int(gallery.nbytes), "selector_bytes": sent, "selector_bytes_plain": plain,
                        "seconds": {"enrol": t_enc - t0, "lookup": t_lookup - t1, "hamming_match": t_match - t_lookup},
                        "levels": {"hamming_match": levels}})
    finally:
        api.set_deferred(was_deferred)
        selector.close()
    return out


def run_inner_product(params, key, templates, probe, tau, width=128, seeded_selectors=False):
    """Client and server of identify.match_by_inner once: the client enrols the gallery (pack_gallery_inner) and sends the
    probe (hamming_probe); the server answers one match bit per template; the client decrypts.  Yields one record per
    template: its distance, the plaintext decision, the decrypted one and whether the distance lies inside the computed
    band around tau where the decision is not guaranteed, and the probe's bytes on the wire beside the plain figure.
    seeded_selectors: the probe travels as a seed-compressed record."""
    from . import identify
    gallery = identify.pack_gallery_inner(templates, width, key)          # client, at enrolment
    tgsw, addend = identify.hamming_probe(probe, width, key, compressed=seeded_selectors)      # client, per query
    selector = api.Selector.from_compressed(params, tgsw) if seeded_selectors else api.Selector(params, tgsw)    # server
    bits = identify.match_by_inner(selector, gallery, len(templates), width, addend, tau, key)
    got = [int(b) for b in bits.decrypt(key)]                             # client
    g = identify.inner_decision_band(params, width)
    for i, t in enumerate(templates):
        d = sum(int(x) ^ int(y) for x, y in zip(t, probe))
        yield {"entry": i, "distance": d, "plain": int(d <= tau), "decrypted": got[i], "inside_band": abs(d - tau) < g,
               "probe_bytes": int(tgsw.nbytes), "probe_bytes_plain": 4 * api.tgsw_words(params)}
    selector.close()
    for o in (bits, addend):
        o.close()


def run_clear_gallery(params, key, templates, probe, tau, width=128):
    """Client and server of identify.match_clear_gallery once: the server owns the gallery in the clear
    (clear_gallery_polys, api.PublicGallery -- nothing is enrolled under a key); the client sends ONE seed-compressed ring
    sample and the addend (hamming_probe_ring); the server answers one match bit per template; the client decrypts.
    Yields run_inner_product's records, plus the probe's bytes on the wire."""
    from . import identify
    gallery = api.PublicGallery(params, identify.clear_gallery_polys(templates, width, params.N))    # server
    ring, addend = identify.hamming_probe_ring(probe, width, key, compressed=True)                   # client, per query
    bits = identify.match_clear_gallery(gallery, ring, len(templates), width, addend, tau, key)
    got = [int(b) for b in bits.decrypt(key)]                             # client
    g = identify.inner_decision_band(params, width)
    for i, t in enumerate(templates):
        d = sum(int(x) ^ int(y) for x, y in zip(t, probe))
        yield {"entry": i, "distance": d, "plain": int(d <= tau), "decrypted": got[i], "inside_band": abs(d - tau) < g,
               "probe_bytes": int(ring.nbytes)}
    gallery.close()
    for o in (bits, addend):
        o.close()


def run_clear_gallery_long(params, key, templates, probe, tau, width=1024, terms=2):
    """run_clear_gallery for templates of terms * width bits (identify.match_clear_gallery_long): the gallery is groups of
    `terms` public polynomials, the client sends `terms` ring samples and the addend; ONE summed product launch, one key
    switch and one bootstrap per template.  Yields run_inner_product's records, plus the probe's bytes on the wire."""
    from . import identify
    gallery = api.PublicGallery(params, identify.clear_gallery_polys_long(templates, width, params.N, terms))    # server
    ring, addend = identify.hamming_probe_ring_long(probe, width, terms, key)                                    # client, per query
    bits = identify.match_clear_gallery_long(gallery, ring, terms, len(templates), width, addend, tau, key)
    got = [int(b) for b in bits.decrypt(key)]                             # client
    g = identify.clear_decision_band(params, identify.inner_delta(terms * width))
    for i, t in enumerate(templates):
        d = sum(int(x) ^ int(y) for x, y in zip(t, probe))
        yield {"entry": i, "distance": d, "plain": int(d <= tau), "decrypted": got[i], "inside_band": abs(d - tau) < g,
               "probe_bytes": int(ring.nbytes)}
    gallery.close()
    for o in (bits, addend):
        o.close()


def run_masked_clear_gallery(params, key, codes, masks, probe, probe_mask, num, den, width=1024):
    """Client and server of identify.match_clear_gallery_masked once: the server owns codes and validity masks in the clear,
    with the threshold num / den folded into its polynomials (masked_gallery_polys); the client sends two ring samples per
    chunk of `width` bits (masked_probe_ring) and NO addend; the server answers one match bit per template -- one row, one
    key switch, one bootstrap each.  Yields one record per template: valid and disagreeing bits, D, the plaintext
    decision, the decrypted one and whether D lies inside the computed band."""
    from . import identify
    length = len(probe)
    gallery = api.PublicGallery(params, identify.masked_gallery_polys(codes, masks, width, params.N, num, den))  # server
    ring = identify.masked_probe_ring(probe, probe_mask, width, num, den, key)                                   # client, per query
    bits = identify.match_clear_gallery_masked(gallery, ring, len(codes), width, length, num, den, key)
    got = [int(b) for b in bits.decrypt(key)]                             # client
    g = identify.clear_decision_band(params, identify.masked_delta(den, length))
    for i, (code, mask) in enumerate(zip(codes, masks)):
        valid = sum(int(m) & int(n) for m, n in zip(probe_mask, mask))
        disagree = sum((int(x) ^ int(y)) & int(m) & int(n) for x, y, m, n in zip(probe, code, probe_mask, mask))
        D = identify.masked_decision(probe, code, probe_mask, mask, num, den)
        yield {"entry": i, "valid": valid, "disagree": disagree, "D": D, "plain": int(den * disagree <= num * valid),
               "decrypted": got[i], "inside_band": abs(D) < g, "probe_bytes": int(ring.nbytes)}
    gallery.close()
    bits.close()


def run_inner_product_long(params, key, templates, probe, tau, width=1024, terms=2, seeded_selectors=False):
    """run_inner_product for templates of terms * width bits against an ENCRYPTED gallery (identify.match_by_inner_long): the
    gallery is enrolled as groups of `terms` ring samples, the client sends the `terms` TGSW probe polynomials as ONE selector
    record (seed-compressed with seeded_selectors) and the addend; ONE summed product launch, one key switch and one
    bootstrap per template.  Yields run_inner_product's records."""
    from . import identify
    gallery = identify.pack_gallery_inner_long(templates, width, terms, key)                                     # client, at enrolment
    tgsw, addend = identify.hamming_probe_long(probe, width, terms, key, compressed=seeded_selectors)            # client, per query
    selector = api.Selector.from_compressed(params, tgsw) if seeded_selectors else api.Selector(params, tgsw)   # server
    bits = identify.match_by_inner_long(selector, gallery, terms, len(templates), width, addend, tau, key)
    got = [int(b) for b in bits.decrypt(key)]                             # client
    g = identify.inner_sum_decision_band(params, identify.inner_delta(terms * width), terms)
    for i, t in enumerate(templates):
        d = sum(int(x) ^ int(y) for x, y in zip(t, probe))
        yield {"entry": i, "distance": d, "plain": int(d <= tau), "decrypted": got[i], "inside_band": abs(d - tau) < g,
               "probe_bytes": int(tgsw.nbytes), "probe_bytes_plain": 4 * terms * api.tgsw_words(params)}
    selector.close()
    for o in (bits, addend):
        o.close()


def run_masked_inner_product(params, key, codes, masks, probe, probe_mask, num, den, width=1024, seeded_selectors=False):
    """Client and server of identify.match_by_inner_masked once: codes and validity masks are enrolled ENCRYPTED, with the
    threshold num / den folded into the messages (masked_gallery_inner); the client sends two 0 / +-1 TGSW probe polynomials
    per chunk of `width` bits as ONE selector record (masked_probe_tgsw) and NO addend; the server answers one match bit per
    template -- one row, one key switch, one bootstrap each.  Yields run_masked_clear_gallery's records."""
    from . import identify
    length = len(probe)
    gallery = identify.masked_gallery_inner(codes, masks, width, num, den, key)                                  # client, at enrolment
    tgsw = identify.masked_probe_tgsw(probe, probe_mask, width, num, den, key, compressed=seeded_selectors)      # client, per query
    selector = api.Selector.from_compressed(params, tgsw) if seeded_selectors else api.Selector(params, tgsw)   # server
    bits = identify.match_by_inner_masked(selector, gallery, len(codes), width, length, num, den, key)
    got = [int(b) for b in bits.decrypt(key)]                             # client
    g = identify.masked_inner_band(params, length, width, den)
    for i, (code, mask) in enumerate(zip(codes, masks)):
        valid = sum(int(m) & int(n) for m, n in zip(probe_mask, mask))
        disagree = sum((int(x) ^ int(y)) & int(m) & int(n) for x, y, m, n in zip(probe, code, probe_mask, mask))
        D = identify.masked_decision(probe, code, probe_mask, mask, num, den)
        yield {"entry": i, "valid": valid, "disagree": disagree, "D": D, "plain": int(den * disagree <= num * valid),
               "decrypted": got[i], "inside_band": abs(D) < g, "probe_bytes": int(tgsw.nbytes)}
    selector.close()
    bits.close()


def run_ring_lut(params, key, table, perm):
    """An ENCRYPTED 8-entry table of 2-bit values looked up under an index the SERVER computed (include/tfhe_hip.h "ring LUT
    bootstrap").  Client: the table as ONE ring sample, entry m on the block of N / 8 coefficients from m N / 8 at phase
    (2 v + 1) / 16, and a 3-bit digit x as a fresh sample at phase (x + 1/2) / 16.  Server: index = perm[x] by a LUT bootstrap
    of the digit (the server's own public function; the result is an LWE sample it computed, recorded, not flushed), then
    api.ring_lut_bootstrap of the table by that index -- the call flushes the recording its input depends on.  Client:
    decrypts the 2-bit value.  Yields one record per digit x = 0 .. 7."""
    import numpy as np
    N = params.N
    mu = np.repeat((2 * np.asarray(table, dtype=np.int64) + 1) << 28, N // 8)
    mu = (mu - ((mu >> 31) << 32)).astype(np.int32)
    ring = api.ring_encrypt(mu, key)                                       # client, once: 8 KB
    xs = api.CiphertextArray(params, 8)
    for x in range(8):
        api.encrypt_torus(xs.at(x), (2 * x + 1) << 27, key)                # client, per query
    lut = api.Lut(params, np.array([(2 * perm[j * 8 // N] + 1) << 27 for j in range(N)], dtype=np.int64).astype(np.int32))
    index, out = api.CiphertextArray(params, 8), api.CiphertextArray(params, 8)
    was = api.get_deferred()
    api.set_deferred(True)
    try:
        api.lut_bootstrap_batch(lut, index, [xs], [1], 0, key)             # server: index = perm[x]
        api.ring_lut_bootstrap(ring.reshape(1, -1), index, key, out, ring_index=[0] * 8)
    finally:
        api.set_deferred(was)
    w = out.words().astype(np.int64)                                       # client
    ph = (w[:, -1] - (w[:, :-1] % 2 ** 32) @ np.asarray(key.lwe_key(), dtype=np.int64)) % 2 ** 32
    for x in range(8):
        yield {"x": x, "index": int(perm[x]), "plain": int(table[perm[x]]), "decrypted": int(ph[x] >> 29), "table_bytes": int(ring.nbytes)}
    lut.close()
    for o in (xs, index, out):
        o.close()


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nslots", type=int, default=128)
    ap.add_argument("--bound", type=int, default=256)
    ap.add_argument("--seed", type=lambda v: int(v, 0), default=0x5EBA1)
    ap.add_argument("--fast", action="store_true", help="Function_f through the optimised DAG (circuits_fast.cpp)")
    ap.add_argument("--clients", type=int, default=0,
                    help="K > 0: K clients with key pairs of their own, Function_f and Function_g batched over them")
    ap.add_argument("--compressed-keys", action="store_true",
                    help="each client ships a seed-compressed cloud key; the server expands it on the device at first use")
    ap.add_argument("--seeded-inputs", action="store_true",
                    help="template and sample travel as seed-compressed ring samples and are opened on the device")
    ap.add_argument("--seeded-lwe", action="store_true",
                    help="template and sample travel as one seed-compressed LWE record each and are opened on the device")
    ap.add_argument("--packed-gallery", action="store_true",
                    help="Hamming match of one claimed identity against a gallery of 128-bit templates packed eight to a ring "
                         "sample: looked up under TGSW-encrypted index bits, the server does not learn which")
    ap.add_argument("--entries", type=int, default=20, help="--packed-gallery, --inner-product, --clear-gallery: templates in the gallery")
    ap.add_argument("--inner-product", action="store_true",
                    help="Hamming 1-to-N of one probe against the whole packed gallery by encrypted inner products: one external "
                         "product per ring sample, one key switch, one level of bootstraps (not exact near the threshold)")
    ap.add_argument("--clear-gallery", action="store_true",
                    help="--inner-product with the roles exchanged: the server owns the gallery in the clear, the probe travels "
                         "as one seed-compressed ring sample; a ring sample times public polynomials, no TGSW sample")
    ap.add_argument("--clear-gallery-long", action="store_true",
                    help="--clear-gallery for 2,048-bit templates: two public polynomials a template, two ring samples a probe, "
                         "one summed product launch (public products over several ring samples)")
    ap.add_argument("--masked-clear-gallery", action="store_true",
                    help="masked 2,048-bit templates at the fractional threshold 8/25 over the bits both masks keep: the weights "
                         "live in the gallery polynomials, one key switch and one bootstrap a template, no addend sample")
    ap.add_argument("--inner-product-long", action="store_true",
                    help="--inner-product for 2,048-bit templates against an encrypted gallery: two ring samples a template, two "
                         "TGSW probe polynomials in one selector record, one summed product launch (TGSW products over several "
                         "ring samples); goes with --seeded-selectors")
    ap.add_argument("--masked-inner-product", action="store_true",
                    help="masked 2,048-bit templates at the fractional threshold 8/25 against an encrypted gallery: the weights live "
                         "in the gallery's messages, four 0/+-1 TGSW probe polynomials, one key switch and one bootstrap a template, "
                         "no addend sample; goes with --seeded-selectors")
    ap.add_argument("--seeded-selectors", action="store_true",
                    help="index bits and TGSW probes travel as seed-compressed records (a seed and the bodies, half the bytes), "
                         "the masks written on the card; alone: the select, the packed lookup and the inner products in turn; "
                         "with --packed-gallery or --inner-product: that route")
    ap.add_argument("--ring-lut", action="store_true",
                    help="an encrypted 8-entry table of 2-bit values looked up under an index the server computed by a LUT "
                         "bootstrap (ring LUT bootstrap: the blind rotation of an encrypted ring sample by an LWE sample); runs alone")
    a = ap.parse_args(argv)
    if a.ring_lut and (a.clients or a.seeded_inputs or a.seeded_lwe or a.fast or a.packed_gallery or a.compressed_keys or a.inner_product or
                       a.clear_gallery or a.clear_gallery_long or a.masked_clear_gallery or a.inner_product_long or
                       a.masked_inner_product or a.seeded_selectors):
        ap.error("--ring-lut runs alone")
    if a.seeded_selectors and (a.clients or a.seeded_inputs or a.seeded_lwe or a.fast or a.clear_gallery):
        ap.error("--seeded-selectors goes with the select, --packed-gallery, --inner-product, --inner-product-long and "
                 "--masked-inner-product only")
    for flag, on in (("--inner-product-long", a.inner_product_long), ("--masked-inner-product", a.masked_inner_product)):
        if on and (a.clients or a.seeded_inputs or a.seeded_lwe or a.fast or a.packed_gallery or a.compressed_keys or a.inner_product or
                   a.clear_gallery or a.clear_gallery_long or a.masked_clear_gallery or (a.inner_product_long and a.masked_inner_product)):
            ap.error(flag + " runs alone or with --seeded-selectors")
        if on and not 1 <= a.entries <= 1 << 16:
            ap.error("--entries must be in 1..2^16")
    if a.seeded_selectors and a.compressed_keys and not a.packed_gallery:
        ap.error("--seeded-selectors takes --compressed-keys with --packed-gallery only")
    if a.seeded_selectors and not 1 <= a.entries <= 1 << 20:
        ap.error("--entries must be in 1..2^20")
    for flag, on in (("--clear-gallery-long", a.clear_gallery_long), ("--masked-clear-gallery", a.masked_clear_gallery)):
        if on and (a.clients or a.seeded_inputs or a.seeded_lwe or a.fast or a.packed_gallery or a.compressed_keys or a.inner_product or
                   a.clear_gallery or a.seeded_selectors or (a.clear_gallery_long and a.masked_clear_gallery)):
            ap.error(flag + " runs alone")
        if on and not 1 <= a.entries <= 1 << 16:
            ap.error("--entries must be in 1..2^16")
    if a.clear_gallery and (a.clients or a.seeded_inputs or a.seeded_lwe or a.fast or a.packed_gallery or a.compressed_keys or a.inner_product):
        ap.error("--clear-gallery runs alone")
    if a.clear_gallery and not 1 <= a.entries <= 1 << 20:
        ap.error("--entries must be in 1..2^20")
    if a.inner_product and (a.clients or a.seeded_inputs or a.seeded_lwe or a.fast or a.packed_gallery or a.compressed_keys):
        ap.error("--inner-product runs alone")
    if a.inner_product and not 1 <= a.entries <= 1 << 20:
        ap.error("--entries must be in 1..2^20")
    if a.packed_gallery and (a.clients or a.seeded_inputs or a.seeded_lwe or a.fast):
        ap.error("--packed-gallery runs the single-client Hamming match alone")
    if a.packed_gallery and not 1 <= a.entries <= 1 << 20:
        ap.error("--entries must be in 1..2^20")
    if a.seeded_lwe and (a.clients or a.seeded_inputs):
        ap.error("--seeded-lwe runs the single-client form, without --seeded-inputs")
    if a.clients < 0:
        ap.error("--clients must be >= 0")
    if a.seeded_inputs and a.clients:
        ap.error("--seeded-inputs runs the single-client form")
    if a.seeded_inputs and a.nslots * 8 > 1024:
        ap.error("--seeded-inputs carries nslots * 8 bits in one ring sample of 1,024")
    return a


def shipped_cloud(key):
    """What --compressed-keys puts between client and server: the client makes a compressed cloud key for its secret
    keyset (40 bytes of seed and the bodies), the server expands it -- the masks are written on the device at first use."""
    ck = api.CompressedCloudKey.generate(key)
    try:
        return api.CompressedCloudKey.from_words(key.params, ck.seed(), ck.bk_body(), ck.ksk_body()).expand()
    finally:
        ck.close()


def main_clients(a):
    params = api.ParameterSet(128)
    inputs = [client_inputs(c, a.nslots, a.seed) for c in range(a.clients)]
    keys = [api.SecretKeySet(params, x["key_seed"], device=not a.compressed_keys) for x in inputs]
    clouds = [shipped_cloud(k) for k in keys] if a.compressed_keys else None
    try:
        outs = run_p1_clients(params, keys, [x["sample"] for x in inputs], [x["template"] for x in inputs],
                              [a.bound] * a.clients, [x["r0"] for x in inputs], [x["r1"] for x in inputs], fast=a.fast,
                              clouds=clouds)
        for x, out in zip(inputs, outs):
            out["distance"] = sum((s - t) ** 2 for s, t in zip(x["sample"], x["template"]))
            print(json.dumps(out))
    finally:
        for k in (clouds or []) + keys:
            k.close()


def main():
    a = parse_args()
    if a.clients:
        return main_clients(a)
    params = api.ParameterSet(128)
    key = api.SecretKeySet(params, a.seed + 1, device=not a.compressed_keys)
    cloud = shipped_cloud(key) if a.compressed_keys else None
    if a.ring_lut:
        import random
        rnd = random.Random(a.seed)
        table = [rnd.getrandbits(2) for _ in range(8)]
        perm = list(range(8))
        rnd.shuffle(perm)
        for out in run_ring_lut(params, key, table, perm):
            print(json.dumps(out))
        key.close()
        return
    long_routes = a.inner_product_long or a.masked_inner_product
    routes = a.seeded_selectors and not (a.packed_gallery or a.inner_product or long_routes)      # alone: the three routes in turn
    if a.clear_gallery_long or a.masked_clear_gallery or long_routes:
        import random
        rnd = random.Random(a.seed)
        length = 2048
        probe = [rnd.getrandbits(1) for _ in range(length)]
        templates = []
        for i in range(a.entries):                                        # every third template near the probe
            t = list(probe) if i % 3 == 0 else [rnd.getrandbits(1) for _ in range(length)]
            for j in rnd.sample(range(length), (97 * i) % 397):
                t[j] ^= 1
            templates.append(t)
        if a.clear_gallery_long:
            outs = run_clear_gallery_long(params, key, templates, probe, tau=655)
        elif a.inner_product_long:
            outs = run_inner_product_long(params, key, templates, probe, tau=655, seeded_selectors=a.seeded_selectors)
        else:
            masks = [[int(rnd.random() < 0.85) for _ in range(length)] for _ in range(a.entries)]
            probe_mask = [int(rnd.random() < 0.9) for _ in range(length)]
            run = run_masked_clear_gallery
            if a.masked_inner_product:
                run = lambda *args, **kw: run_masked_inner_product(*args, seeded_selectors=a.seeded_selectors, **kw)    # noqa: E731
            outs = run(params, key, templates, masks, probe, probe_mask, num=8, den=25)
        for out in outs:
            print(json.dumps(out))
        key.close()
        return
    if routes:
        import random
        rnd = random.Random(a.seed)
        entries = min(a.entries, 64)                                      # (one ring sample per template here)
        templates = [[rnd.getrandbits(8) for _ in range(4)] for _ in range(entries)]
        print(json.dumps(run_private_select(params, key, templates, entries * 2 // 3, seeded_selectors=True)))
    if a.inner_product or a.clear_gallery or routes:
        import random
        rnd = random.Random(a.seed)
        probe = [rnd.getrandbits(1) for _ in range(128)]
        templates = []
        for i in range(a.entries):                                        # every third template near the probe
            t = list(probe) if i % 3 == 0 else [rnd.getrandbits(1) for _ in range(128)]
            for j in rnd.sample(range(128), (5 * i) % 29):
                t[j] ^= 1
            templates.append(t)
        if a.clear_gallery:
            outs = run_clear_gallery(params, key, templates, probe, tau=40)
        else:
            outs = run_inner_product(params, key, templates, probe, tau=40, seeded_selectors=a.seeded_selectors)
        for out in outs:
            print(json.dumps(out))
        if not routes:
            key.close()
            return
    if a.packed_gallery or routes:
        import random
        rnd = random.Random(a.seed)
        templates = [[rnd.getrandbits(1) for _ in range(128)] for _ in range(a.entries)]
        claimed = a.entries * 2 // 3
        genuine = list(templates[claimed])
        for j in rnd.sample(range(128), 5):
            genuine[j] ^= 1
        probes = {"genuine": genuine, "impostor": [rnd.getrandbits(1) for _ in range(128)]}
        for out in run_packed_gallery(params, key, templates, claimed, probes, bound=20, cloud=cloud,
                                      seeded_selectors=a.seeded_selectors):
            print(json.dumps(out))
        if cloud is not None:
            cloud.close()
        key.close()
        return
    template = [(37 * i + 11) % 255 for i in range(a.nslots)]             # SURVEY 8c inputs
    runs = {"genuine": [t + 1 for t in template], "impostor": [(91 * i + 5) % 256 for i in range(a.nslots)]}
    for name, sample in runs.items():
        out = run_p1(params, key, sample, template, a.bound, r0=17, r1=99, cloud=cloud,
                     function_f=circuits.function_f_fast if a.fast else None, seeded_inputs=a.seeded_inputs,
                     seeded_lwe=a.seeded_lwe)
        out["distance"] = sum((x - y) ** 2 for x, y in zip(sample, template))
        print(json.dumps({"run": name, **out}))
    if cloud is not None:
        cloud.close()
    key.close()


if __name__ == "__main__":
    main()
