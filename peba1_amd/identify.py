"""1-to-N identification (BASELINE.json configs[3]): one encrypted probe against M enrolled
templates, i.e. M independent runs of the reference's Function_f (Math.cpp:379-387; the loop a
server would put around main.cpp:533-542, one call per enrolled client).

Matches are independent, so they shard across GPUs with no data-path collective (rank r takes
templates r, r + world, ...; bench.py --mode identify) and, on one GPU, they are recorded
`group` at a time: a flush runs the pending gates of the whole group level by level -- the narrow
tail levels of one match (~80 gates wide) are filled by the other matches of the group -- and
releases their slots, so device memory is bounded by `group`, not by M (one pending Function_f
pins ~0.22 M ciphertext slots of a pool that may grow to 4 M slots).

Only the match-bit ciphertext of each match is kept: M x (n+1) words, the one thing that leaves
the GPU.  Plumbing only: every gate runs in libtfhe-hip.
"""
import numpy as np

from . import api, circuits
from . import lib as _l


def synthetic_template(base, k):
    """Template k of the synthetic gallery used by bench.py and the tests (k = 0: `base`)."""
    return [(v + 29 * k + 3 * i) % 256 if k else v for i, v in enumerate(base)]


def identify(params, key, probe, templates, bound, bitsize, group=4, on_group=None, circuit=None, comm=None, all_bits=None):
    """Returns a CiphertextArray of len(templates) match-bit ciphertexts: element m encrypts
    (distance(probe, templates[m]) > bound), the reference's polarity.

    probe, templates[m]: circuits.EncryptedVector; bound: 3*bitsize-sample number.
    `group` matches are recorded per flush.  The loop itself is host C++ (libpeba1-dist peba1_identify, VERDICT r3
    item 5: a C++ server reaches configs[3] with no Python in the process); this is its thin caller.
    `comm` (a dist.Comm) + `all_bits` (rank 0: a CiphertextArray of world * len(templates) samples): the match bits of
    every rank are gathered to rank 0 by the same call.
    `circuit`: circuits.function_f (default, the reference's gate sequence) or function_f_fast.
    `on_group(first, count)`: called after each group; given one, the groups are driven from here, one C call each."""
    from . import dist as pd
    circuits.load()                       # libpeba1-circuits, RTLD_GLOBAL: libpeba1-dist resolves the circuits there
    _l.load()
    fast = circuit is circuits.function_f_fast
    if circuit is not None and not fast and circuit is not circuits.function_f:
        raise ValueError("identify runs circuits.function_f or circuits.function_f_fast")
    M = len(templates)
    nslots = len(probe.slots)
    bits = api.CiphertextArray(params, M)
    P = [a.ptr for a in probe.slots]
    if on_group is None:
        T = [a.ptr for t in templates for a in t.slots]
        pd.identify(comm, all_bits.ptr if all_bits is not None else None, bits.ptr, P, T, nslots, bound.ptr, bitsize,
                    key.cloud, group=group, fast=fast)
        return bits
    for first in range(0, M, group):
        count = min(group, M - first)
        T = [a.ptr for t in templates[first:first + count] for a in t.slots]
        pd.identify(None, None, bits.at(first), P, T, nslots, bound.ptr, bitsize, key.cloud, group=group, fast=fast)
        on_group(first, count)
    if comm is not None:
        pd.gather_samples(comm, all_bits.ptr if all_bits is not None else None, bits.ptr, M, params.ptr)
    return bits


def pack_match_bits(pkey, bits, key):
    """The match bits identify() returned, packed for the way back (api.pack): one ring sample of (k+1) N words per N
    match bits instead of n + 1 words per bit.  Returns [(words, count), ...], one entry per started N bits;
    api.packed_decrypt(words, count, secret) gives the bits back on the client."""
    N = pkey.params.N
    return [(api.pack(pkey, bits, min(N, bits.count - first), key, first=first), min(N, bits.count - first))
            for first in range(0, bits.count, N)]


def unpack_templates(ring_words_list, params, nslots, bitsize, key):
    """The way in for a gallery that travels and rests as ring samples: one EncryptedVector per entry of ring_words_list
    (each the (k+1) N words circuits.ring_encrypt_vector made on the client, or the 10 + N words of its compressed form --
    told apart by their count -- in which a gallery rests in half the bytes), ready for identify().  One unpack per
    template; LWE samples exist only on the device."""
    return [circuits.EncryptedVector.from_ring(params, w, nslots, bitsize, key) for w in ring_words_list]


def select_template(selector, ring_gallery, params, nslots, bitsize, key):
    """Verification against a claimed identity the server must not learn: the CMUX tree of `selector` (api.Selector over
    the client's TGSW-encrypted index bits) picks one template of a gallery that rests as ring samples, and the selected
    sample is opened like any template that arrived as one (EncryptedVector.from_ring), ready for function_f.  ring_gallery:
    [M][(k+1) N] host words, or an int32 torch tensor resident on the device -- then only the (k+1) N selected words pass
    through the host on their way into the unpack, the gallery stays where it is."""
    device = hasattr(ring_gallery, "data_ptr")               # a torch tensor; anything else is host words
    words = api.ring_select(selector, ring_gallery, device=device)
    if device:
        if _l.load().tfhe_hip_stream_sync() != 0:
            raise RuntimeError(api.last_error())
        words = words.cpu().numpy()
    return circuits.EncryptedVector.from_ring(params, words, nslots, bitsize, key)


def pack_gallery(entries, width, secret, compressed=False, seed=None, mask_seed=None):
    """The client side of lookup_template: M entries of `width` bits each (width a power of two up to N), S = N / width of
    them per ring sample under the secret keyset `secret` -- bit j of entry i at coefficient (i mod S) width + j of sample
    i / S (api.ring_encrypt_bits; a last sample that is not full carries 0 behind its entries).  A gallery of 128-bit
    templates rests at 1 KB per template at N = 1,024 where select_template's rests at 8 KB.  Returns int32 [R][(k+1) N],
    R = ceil(M / S); compressed: [R][10 + N], which api.ring_expand turns into the former on the server.  seed (and
    mask_seed, compressed): the reproducible form, sample r drawn from seed + r."""
    N = secret.params.N
    R = api.lookup_samples(secret.params, len(entries), width)
    S = N // width
    out = []
    for r in range(R):
        bits = []
        for e in entries[r * S:(r + 1) * S]:
            e = [int(b) & 1 for b in e]
            if len(e) != width:
                raise ValueError("every entry carries %d bits" % width)
            bits += e
        out.append(api.ring_encrypt_bits(bits, secret, seed=None if seed is None else seed + r, compressed=compressed,
                                         mask_seed=mask_seed))
    return np.stack(out)


def lookup_template(selector, ring_gallery, M, width, key):
    """select_template's packed twin: api.ring_lookup of `selector` over a gallery pack_gallery made (host words
    [R][(k+1) N], or an int32 torch tensor resident on the device), then the unpack of coefficients 0 .. width - 1 of the
    result: a CiphertextArray of the `width` bits of the entry the client's index names, ready for circuits.hamming_match.
    key: the keyset whose cloud key evaluates.  From a resident gallery nothing passes through the host."""
    params = selector.params
    device = hasattr(ring_gallery, "data_ptr")
    words = api.ring_lookup(selector, ring_gallery, M, width, device=device)
    bits = api.CiphertextArray(params, width)
    if device:
        api.unpack_device(words.data_ptr(), 1, key, bits, count=width)
        if _l.load().tfhe_hip_stream_sync() != 0:            # `words` is released on return
            raise RuntimeError(api.last_error())
    else:
        api.unpack(words, key, bits, count=width)
    return bits


# ---- Hamming 1-to-N by encrypted inner products (include/tfhe_hip.h "encrypted inner products") ----
def inner_delta(width):
    """Delta = 2^-(log2 width + 2) as a torus word: `width` disagreeing bits reach 1/4"""
    if width < 1 or width & (width - 1):
        raise ValueError("width must be a power of two")
    return (1 << 30) // width


def inner_round_gallery(words, params):
    """Every word of ring samples + 2^(31 - l Bgbit), wrapping (tfhe_hip_ring_center_words): half a step of the offset
    decomposition, which keeps the top l Bgbit bits of a word and so errs by [0, 2 eps) -- a MEAN of eps per coefficient that
    a probe of coefficient sum s multiplies by up to s (1 + N / 2) (1.6e-2 at P128 for 128 equal bits).  With the half step
    in place the kept digits are those of the rounded word and the error is the zero-mean [-eps, eps) the header's rounding
    term assumes.  A public operation on ciphertext words: client or server may apply it, once.  Returns a copy."""
    w = np.ascontiguousarray(words, dtype=np.int32).copy()
    flat = w.reshape(-1)
    if _l.load().tfhe_hip_ring_center_words(params.ptr, api._i32p(flat), flat.size) != 0:
        raise RuntimeError(api.last_error())
    return w


def pack_gallery_inner(entries, width, secret, seed=None):
    """Enrolment for match_by_inner: M entries of `width` bits each in pack_gallery's layout (S = N / width per ring sample,
    bit j of entry i at coefficient (i mod S) width + j of sample i / S), a bit of 1 carried at amplitude Delta =
    2^-(log2 width + 2) and a bit of 0 as 0 (api.ring_encrypt), the words then centred for the decomposition
    (inner_round_gallery).  Returns int32 [R][(k+1) N]; seed: the reproducible form, sample r drawn from seed + r."""
    N = secret.params.N
    R = api.lookup_samples(secret.params, len(entries), width)
    S, delta = N // width, inner_delta(width)
    out = []
    for r in range(R):
        mu = np.zeros(N, dtype=np.int64)
        for e, entry in enumerate(entries[r * S:(r + 1) * S]):
            bits = [int(b) & 1 for b in entry]
            if len(bits) != width:
                raise ValueError("every entry carries %d bits" % width)
            mu[e * width:(e + 1) * width] = np.asarray(bits, dtype=np.int64) * delta
        out.append(api.ring_encrypt(mu.astype(np.int32), secret, seed=None if seed is None else seed + r))
    return inner_round_gallery(np.stack(out), secret.params)


def hamming_probe_poly(bits, N):
    """sum_i s_i X^(-i) with s_i = 1 - 2 b_i: p[0] = s_0, p[N - i] = -s_i -> int32 [N]"""
    s = 1 - 2 * (np.asarray(bits, dtype=np.int64).reshape(-1) & 1)
    if not 1 <= len(s) <= N:
        raise ValueError("a probe carries 1..%d bits" % N)
    p = np.zeros(N, dtype=np.int32)
    p[0] = s[0]
    for i in range(1, len(s)):
        p[N - i] = -s[i]
    return p


def hamming_probe(bits, width, secret, seed=None, compressed=False):
    """The client's probe for match_by_inner over a gallery of `width`-bit entries: (the TGSW words of sum_i (1 - 2 b_i)
    X^(-i), ready for api.Selector, and a CiphertextArray of ONE sample that encrypts (sum_i b_i) Delta, the addend that turns
    the inner product into the Hamming distance; Delta is the gallery's, 2^-(log2 width + 2)).  len(bits) must be `width`.
    seed: the reproducible TGSW form.  compressed: the probe as a seed-compressed record instead (10 + (k+1) l N words, half
    the bytes), ready for api.Selector.from_compressed."""
    params = secret.params
    b = np.asarray(bits, dtype=np.int64).reshape(-1) & 1
    if len(b) != width:
        raise ValueError("the probe carries %d bits, the gallery's entries %d" % (len(b), width))
    encrypt = api.tgsw_encrypt_polys_compressed if compressed else api.tgsw_encrypt_polys
    words = encrypt(hamming_probe_poly(b, params.N)[None, :], secret, seed=seed)
    addend = api.CiphertextArray(params, 1)
    api.encrypt_torus(addend.at(0), int(b.sum()) * inner_delta(width), secret)
    return words, addend


def inner_decision_sigma(params):
    """sigma_dec of the header, COMPUTED (torus units): the unpack's key switch, N t ks_stdev^2 + (N / 2) prec^2 / 3, plus
    the bootstrap's modulus switch, (1 + n / 2) / (12 (2N)^2)"""
    ks_stdev = params.ptr.contents.in_out_params.contents.alpha_min
    N, n = params.N, params.n
    prec = 2.0 ** -(1 + params.ks_basebit * params.ks_t)
    return (N * params.ks_t * ks_stdev ** 2 + (N / 2.0) * prec ** 2 / 3.0 + (1.0 + n / 2.0) / (12.0 * (2.0 * N) ** 2)) ** 0.5


def inner_decision_band(params, width):
    """The smallest integer g with (g - 1/2) Delta >= 6 sigma_dec: match_by_inner's answer for an entry at distance d is
    guaranteed only where |d - tau| >= g.  12 at P128 and width 128, 2 at width 16."""
    delta = inner_delta(width) / 2.0 ** 32
    g = 1
    while (g - 0.5) * delta < 6.0 * inner_decision_sigma(params):
        g += 1
    return g


def match_by_inner(selector, gallery, M, width, addend, tau, key, sample=0):
    """Hamming 1-to-N in one product launch, one key switch and one level of M bootstraps: api.ring_inner of sample
    `sample` of `selector` (hamming_probe's words) over a gallery pack_gallery_inner made (host words, or an int32 torch
    tensor resident on the device), then per entry (tau + 1/2) Delta - (inner + addend) (api.linear, recorded) and the LUT
    bootstrap with the constant 1/8, and one flush.  Returns a CiphertextArray of M match bits, TRUE iff distance <= tau --
    NOT exact within inner_decision_band of the threshold -- ready for pack_match_bits."""
    params = selector.params
    device = hasattr(gallery, "data_ptr")
    inner = api.CiphertextArray(params, M)
    api.ring_inner(selector, sample, gallery, M, width, key, inner, device=device)
    return _hamming_decision(params, inner, M, width, addend, tau, key)


def _hamming_decision(params, inner, M, width, addend, tau, key):
    """The decision tail match_by_inner and match_clear_gallery share: per entry (tau + 1/2) Delta - (inner + addend)
    (api.linear, recorded), the LUT bootstrap with the constant 1/8, one flush.  Closes `inner`."""
    delta = inner_delta(width)
    lin = api.CiphertextArray(params, M)
    c0 = (2 * int(tau) + 1) * delta // 2
    for i in range(M):
        api.linear(lin.at(i), [inner.at(i), addend.at(0)], [-1, -1], c0, key)
    lut = api.Lut.constant(params, 1 << 29)
    bits = api.CiphertextArray(params, M)
    api.lut_bootstrap_batch(lut, bits, [lin], [1], 0, key)
    api.flush()                                               # (the device form's gallery has been read by now)
    lut.close()
    for o in (inner, lin):
        o.close()
    return bits


# ---- Hamming 1-to-N against a CLEAR gallery (include/tfhe_hip.h "ring sample times public polynomials") ----
def clear_gallery_polys(entries, width, N):
    """A gallery the server owns in the clear, as public polynomials for api.PublicGallery: M entries of `width` bits in
    pack_gallery's layout (S = N / width per polynomial, bit j of entry i at coefficient (i mod S) width + j of polynomial
    i / S, 0 behind the last entry) -> int32 [R][N], R = ceil(M / S)."""
    if width < 1 or width > N or width & (width - 1):
        raise ValueError("width must be a power of two in 1..%d" % N)
    S = N // width
    R = -(-len(entries) // S)
    q = np.zeros((max(R, 1), N), dtype=np.int32)
    for i, entry in enumerate(entries):
        bits = [int(b) & 1 for b in entry]
        if len(bits) != width:
            raise ValueError("every entry carries %d bits" % width)
        q[i // S, (i % S) * width:(i % S + 1) * width] = bits
    return q


def hamming_probe_ring(bits, width, secret, compressed=False, seed=None):
    """The client's probe for match_clear_gallery: (ONE ring sample that encrypts the torus polynomial sum_i s_i Delta
    X^(-i), s_i = 1 - 2 b_i, Delta = 2^-(log2 width + 2) -- (k+1) N words, or the 10 + N words of the seed-compressed form --
    and a CiphertextArray of ONE sample that encrypts (sum_i b_i) Delta, hamming_probe's addend).  len(bits) must be
    `width`.  seed: the reproducible form (the compressed form's mask seed is derived from it)."""
    params = secret.params
    b = np.asarray(bits, dtype=np.int64).reshape(-1) & 1
    if len(b) != width:
        raise ValueError("the probe carries %d bits, the gallery's entries %d" % (len(b), width))
    mu = hamming_probe_poly(b, params.N).astype(np.int64) * inner_delta(width)
    mask_seed = None if seed is None or not compressed else [(int(seed) * 0x9E3779B1 + j) & 0xFFFFFFFF for j in range(10)]
    words = api.ring_encrypt(mu, secret, seed=seed, compressed=compressed, mask_seed=mask_seed)
    addend = api.CiphertextArray(params, 1)
    api.encrypt_torus(addend.at(0), int(b.sum()) * inner_delta(width), secret)
    return words, addend


def match_clear_gallery(gallery, probe_ring, M, width, addend, tau, key):
    """match_by_inner with the roles exchanged: `gallery` is an api.PublicGallery over clear_gallery_polys, `probe_ring`
    hamming_probe_ring's sample (host words, plain or seed-compressed -- told apart by their count --, or an int32 torch
    tensor of the plain words resident on the device).  api.ring_inner_public, then match_by_inner's decision tail, word
    for word.  Returns a CiphertextArray of M match bits, TRUE iff distance <= tau -- NOT exact within inner_decision_band
    of the threshold, exactly as match_by_inner: the band is the key switch's and the modulus switch's."""
    params = gallery.params
    device = hasattr(probe_ring, "data_ptr")
    if not device:
        probe_ring = np.ascontiguousarray(probe_ring, dtype=np.int32).reshape(-1)
        if probe_ring.size == 10 + params.N:
            probe_ring = api.ring_expand(probe_ring, params.N)
    inner = api.CiphertextArray(params, M)
    api.ring_inner_public(gallery, probe_ring, M, width, key, inner, device=device)
    return _hamming_decision(params, inner, M, width, addend, tau, key)    # (its flush: the device form's probe has been read)


# ---- long and masked templates against a CLEAR gallery (include/tfhe_hip.h "public products over several ring samples") ----
def clear_decision_band(params, delta):
    """inner_decision_band for any amplitude: the smallest integer g with (g - 1/2) Delta >= 6 sigma_dec, `delta` the torus
    word of Delta.  The decision of a match whose phase is (1/2 - D) Delta (D an integer: d - tau for a Hamming distance,
    the masked route's D) is guaranteed only where |D| >= g, and is NOT exact inside the band.  At inner_delta(128) this
    is inner_decision_band(params, 128) = 12 at P128.  Computed at P128: 184 for long 2,048-bit codes (Delta = 2^-13);
    5,869 in units of D for masked 2,048-bit codes at 8/25 (Delta = 2^-18), 118 disagreeing bits at full validity."""
    d = int(delta) / 2.0 ** 32
    if d <= 0:
        raise ValueError("Delta must be positive")
    six = 6.0 * inner_decision_sigma(params)
    g = max(int(six / d + 0.5) - 1, 1)
    while (g - 0.5) * d < six:
        g += 1
    return g


def probe_layout(values, N):
    """sum_i v_i X^(-i) for integers v_i: p[0] = v_0, p[N - i] = -v_i (hamming_probe_poly for any coefficients) -> int64 [N]"""
    v = np.asarray(values, dtype=np.int64).reshape(-1)
    if not 1 <= len(v) <= N:
        raise ValueError("a probe carries 1..%d coefficients" % N)
    p = np.zeros(N, dtype=np.int64)
    p[0] = v[0]
    p[N - np.arange(1, len(v))] = -v[1:]
    return p


def _long_shape(width, N, terms):
    if width < 1 or width > N or width & (width - 1):
        raise ValueError("width must be a power of two in 1..%d" % N)
    if not 1 <= terms <= api.PUBLIC_MAX_TERMS or terms & (terms - 1):
        raise ValueError("terms must be a power of two in 1..%d" % api.PUBLIC_MAX_TERMS)
    return N // width


def clear_gallery_polys_long(entries, width, N, terms):
    """clear_gallery_polys for entries of terms * width bits: S = N / width entries to a GROUP of `terms` polynomials, term t
    of group i / S holding bits t width .. t width + width - 1 of entry i at coefficients (i mod S) width .. of polynomial
    (i / S) terms + t -> int32 [R terms][N], R = ceil(M / S) groups."""
    S = _long_shape(width, N, terms)
    R = max(-(-len(entries) // S), 1)
    q = np.zeros((R * terms, N), dtype=np.int32)
    for i, entry in enumerate(entries):
        bits = np.asarray([int(b) & 1 for b in entry], dtype=np.int32)
        if len(bits) != terms * width:
            raise ValueError("every entry carries %d bits" % (terms * width))
        for t in range(terms):
            q[(i // S) * terms + t, (i % S) * width:(i % S + 1) * width] = bits[t * width:(t + 1) * width]
    return q


def hamming_probe_ring_long(bits, width, terms, secret, seed=None):
    """The client's probe for match_clear_gallery_long: (`terms` ring samples, sample t encrypting sum_i s_i Delta X^(-i) over
    bits t width .., s_i = 1 - 2 b_i, Delta = 2^-(log2(terms width) + 2) -> int32 [terms][(k+1) N], and a CiphertextArray of
    ONE sample that encrypts (sum_i b_i) Delta over all terms * width bits).  seed: the reproducible form, sample t from
    seed + t."""
    params = secret.params
    _long_shape(width, params.N, terms)
    b = np.asarray(bits, dtype=np.int64).reshape(-1) & 1
    if len(b) != terms * width:
        raise ValueError("the probe carries %d bits, the gallery's entries %d" % (len(b), terms * width))
    delta = inner_delta(terms * width)
    words = np.stack([api.ring_encrypt(probe_layout(1 - 2 * b[t * width:(t + 1) * width], params.N) * delta, secret,
                                       seed=None if seed is None else seed + t) for t in range(terms)])
    addend = api.CiphertextArray(params, 1)
    api.encrypt_torus(addend.at(0), int(b.sum()) * delta, secret)
    return words, addend


def match_clear_gallery_long(gallery, probe_ring, terms, M, width, addend, tau, key):
    """match_clear_gallery for entries of terms * width bits: `gallery` an api.PublicGallery over clear_gallery_polys_long,
    `probe_ring` hamming_probe_ring_long's samples (host words, or an int32 torch tensor resident on the device).
    api.ring_inner_public_sum -- ONE product launch, one key switch per entry --, then the unchanged decision tail with Delta =
    2^-(log2(terms width) + 2) and the addend sample.  TRUE iff distance <= tau; NOT exact within
    clear_decision_band(params, inner_delta(terms * width)) of the threshold."""
    params = gallery.params
    inner = api.CiphertextArray(params, M)
    api.ring_inner_public_sum(gallery, probe_ring, terms, M, width, key, inner, device=hasattr(probe_ring, "data_ptr"))
    return _hamming_decision(params, inner, M, terms * width, addend, tau, key)


def masked_delta(den, length):
    """Delta = 2^-(2 + ceil(log2(den L))) as a torus word: |D| Delta stays below 1/2 for every D of an entry of L bits"""
    if den < 1 or length < 1 or (den * length - 1).bit_length() > 29:
        raise ValueError("den L must be in 1..2^29")
    return 1 << (30 - (int(den) * int(length) - 1).bit_length())


def masked_decision(b, g, m, n, num, den):
    """D = (den - 2 num) valid - den (agree - disagree) over the bits both masks keep, in plain integers: disagree / valid <=
    num / den iff D <= 0 (D = 2 (den disagree - num valid))"""
    b, g, m, n = (np.asarray(x, dtype=np.int64).reshape(-1) & 1 for x in (b, g, m, n))
    return int((den - 2 * num) * (m * n).sum() - den * ((1 - 2 * b) * (1 - 2 * g) * m * n).sum())


def _masked_shape(length, width, N, num, den, max_terms=None):
    """(S, chunks) of masked entries of `length` bits in chunks of `width`; max_terms: the most terms the summed product
    takes, two a chunk (default: the public sum's)"""
    most = api.PUBLIC_MAX_TERMS if max_terms is None else max_terms
    if width < 1 or width > N or width & (width - 1):
        raise ValueError("width must be a power of two in 1..%d" % N)
    if length < width or length % width or 2 * (length // width) > most:
        raise ValueError("an entry carries 1..%d chunks of %d bits" % (most // 2, width))
    if not 0 < num < den:
        raise ValueError("the threshold num / den must lie inside (0, 1)")
    return N // width, length // width


def masked_gallery_polys(codes, masks, width, N, num, den):
    """A masked gallery the server owns in the clear, with the threshold's weights in it: M entries of L = chunks * width
    code bits g and mask bits n (1 = valid), sigma = 1 - 2 g.  Entry i of group i / S (S = N / width) takes, per chunk c, the
    TWO polynomials (i / S) terms + 2 c and + 2 c + 1, terms = 2 chunks: -den sigma_j n_j and (den - 2 num) n_j at
    coefficients (i mod S) width + j -> int32 [R terms][N].  A group's largest coefficients sum to chunks (den + |den - 2
    num|), which the CRT bound holds to public_max_coef(N)."""
    codes, masks = np.asarray(codes, dtype=np.int64) & 1, np.asarray(masks, dtype=np.int64) & 1
    if codes.ndim != 2 or codes.shape != masks.shape:
        raise ValueError("codes and masks are [M][L] bits of one shape")
    S, chunks = _masked_shape(codes.shape[1], width, N, num, den)
    terms = 2 * chunks
    R = max(-(-len(codes) // S), 1)
    q = np.zeros((R * terms, N), dtype=np.int32)
    for i in range(len(codes)):
        sig_n, n = (1 - 2 * codes[i]) * masks[i], masks[i]
        for c in range(chunks):
            at = slice((i % S) * width, (i % S + 1) * width)
            q[(i // S) * terms + 2 * c, at] = -den * sig_n[c * width:(c + 1) * width]
            q[(i // S) * terms + 2 * c + 1, at] = (den - 2 * num) * n[c * width:(c + 1) * width]
    return q


def masked_probe_ring(bits, mask, width, num, den, secret, seed=None):
    """The client's probe for match_clear_gallery_masked: per chunk of `width` bits the TWO ring samples that encrypt s_i m_i
    Delta and m_i Delta in probe layout (s = 1 - 2 b, m the mask, 1 = valid), Delta = masked_delta(den, L) -> int32
    [2 chunks][(k+1) N].  There is no addend sample.  seed: the reproducible form, sample t from seed + t."""
    params = secret.params
    b, m = (np.asarray(x, dtype=np.int64).reshape(-1) & 1 for x in (bits, mask))
    if len(b) != len(m):
        raise ValueError("code and mask carry the same number of bits")
    _, chunks = _masked_shape(len(b), width, params.N, num, den)
    delta = masked_delta(den, len(b))
    polys = []
    for c in range(chunks):
        at = slice(c * width, (c + 1) * width)
        polys += [probe_layout((1 - 2 * b[at]) * m[at], params.N) * delta, probe_layout(m[at], params.N) * delta]
    return np.stack([api.ring_encrypt(mu, secret, seed=None if seed is None else seed + t) for t, mu in enumerate(polys)])


def masked_product_sigma(num, den, valid_bits, bk_stdev):
    """COMPUTED sigma of D Delta before the key switch (torus units): sum_t |q_t|_2^2 = (den^2 + (den - 2 num)^2) per valid
    gallery bit, times the probe samples' variance; nothing else"""
    return ((den ** 2 + (den - 2 * num) ** 2) * valid_bits) ** 0.5 * bk_stdev


def masked_weight_gain(num, den):
    """What applying the weights BEFORE the key switch buys, COMPUTED: the two-product route (valid and agree - disagree as two
    key-switched inner products, weighted by api.linear afterwards) multiplies the key switch's sigma by sqrt(den^2 +
    (den - 2 num)^2) -- 26.6 at 8/25 --; here the key switch's sigma enters once."""
    return float(den ** 2 + (den - 2 * num) ** 2) ** 0.5


def _masked_decision_tail(params, inner, M, delta, key):
    """The decision tail match_clear_gallery_masked and match_by_inner_masked share: per entry Delta / 2 - D Delta (api.linear,
    a constant alone, recorded), the LUT bootstrap with the constant 1/8, one flush.  Closes `inner`."""
    lin = api.CiphertextArray(params, M)
    for i in range(M):
        api.linear(lin.at(i), [inner.at(i)], [-1], delta // 2, key)
    lut = api.Lut.constant(params, 1 << 29)
    bits = api.CiphertextArray(params, M)
    api.lut_bootstrap_batch(lut, bits, [lin], [1], 0, key)
    api.flush()
    lut.close()
    for o in (inner, lin):
        o.close()
    return bits


def match_clear_gallery_masked(gallery, probe_ring, M, width, length, num, den, key):
    """Masked Hamming 1-to-N at the fractional threshold num / den: `gallery` an api.PublicGallery over masked_gallery_polys,
    `probe_ring` masked_probe_ring's samples (host words, or an int32 torch tensor resident on the device), `length` the
    entries' L.  api.ring_inner_public_sum with terms = 2 L / width gives D Delta per entry -- ONE row, one key switch --;
    then Delta / 2 - D Delta (api.linear, a constant alone, recorded: no addend sample), the LUT bootstrap with the constant
    1/8 and one flush: what match_clear_gallery costs per entry.  The weights den and den - 2 num are in the gallery
    polynomials, so they are applied BEFORE the key switch, whose noise then enters once (masked_weight_gain).  Returns a
    CiphertextArray of M match bits, TRUE iff disagree / valid <= num / den -- NOT exact where |D| <
    clear_decision_band(params, masked_delta(den, length))."""
    params = gallery.params
    _, chunks = _masked_shape(length, width, params.N, num, den)
    delta = masked_delta(den, length)
    inner = api.CiphertextArray(params, M)
    api.ring_inner_public_sum(gallery, probe_ring, 2 * chunks, M, width, key, inner, device=hasattr(probe_ring, "data_ptr"))
    return _masked_decision_tail(params, inner, M, delta, key)          # (its flush: the device form's probe has been read)


# ---- long and masked templates against an ENCRYPTED gallery (include/tfhe_hip.h "TGSW products over several ring samples") ----
def _inner_sum_terms(params, terms):
    most = api.inner_sum_max_terms(params)
    if not 1 <= terms <= most:
        raise ValueError("terms must be in 1..%d for this parameter set" % most)


def _long_inner_shape(params, width, terms):
    N = params.N
    if width < 1 or width > N or width & (width - 1):
        raise ValueError("width must be a power of two in 1..%d" % N)
    _inner_sum_terms(params, terms)
    if terms & (terms - 1):
        raise ValueError("terms must be a power of two (Delta = 2^-(log2(terms width) + 2))")
    return N // width


def _encrypt_groups(mu, secret, seed):
    """ring samples of the torus polynomials mu [R][N], sample r from seed + r, centred for the decomposition"""
    out = [api.ring_encrypt(m, secret, seed=None if seed is None else seed + r) for r, m in enumerate(mu)]
    return inner_round_gallery(np.stack(out), secret.params)


def pack_gallery_inner_long(entries, width, terms, secret, seed=None):
    """Enrolment for match_by_inner_long: M entries of terms * width bits, S = N / width entries to a GROUP of `terms` ring
    samples, term t of group i / S holding bits t width .. t width + width - 1 of entry i at coefficients (i mod S) width ..
    (the lookup's layout), a bit of 1 at amplitude Delta = 2^-(log2(terms width) + 2); the words are centred for the
    decomposition (inner_round_gallery).  Returns int32 [R terms][(k+1) N], R = ceil(M / S) groups; seed: the reproducible
    form, sample r drawn from seed + r."""
    params = secret.params
    S = _long_inner_shape(params, width, terms)
    delta = inner_delta(terms * width)
    R = max(-(-len(entries) // S), 1)
    mu = np.zeros((R * terms, params.N), dtype=np.int64)
    for i, entry in enumerate(entries):
        bits = np.asarray([int(b) & 1 for b in entry], dtype=np.int64)
        if len(bits) != terms * width:
            raise ValueError("every entry carries %d bits" % (terms * width))
        for t in range(terms):
            mu[(i // S) * terms + t, (i % S) * width:(i % S + 1) * width] = bits[t * width:(t + 1) * width] * delta
    return _encrypt_groups(mu, secret, seed)


def hamming_probe_long_polys(bits, width, terms, N):
    """the `terms` probe polynomials of hamming_probe_long: polynomial t is sum_i s_i X^(-i) over bits t width .. -> int32 [terms][N]"""
    b = np.asarray(bits, dtype=np.int64).reshape(-1) & 1
    if len(b) != terms * width:
        raise ValueError("the probe carries %d bits, the gallery's entries %d" % (len(b), terms * width))
    return np.stack([probe_layout(1 - 2 * b[t * width:(t + 1) * width], N) for t in range(terms)]).astype(np.int32)


def hamming_probe_rounding_weight(bits, width, terms, N):
    """sum_t probe_rounding_weight of the `terms` probe polynomials of a code: what the client puts into
    inner_sum_decision_band for the band of ITS probe (random-looking codes stay inside the default (1 + N) terms width)"""
    b = np.asarray(bits, dtype=np.int64).reshape(-1) & 1
    if len(b) != terms * width:
        raise ValueError("the probe carries %d bits, the gallery's entries %d" % (len(b), terms * width))
    return sum(probe_rounding_weight(1 - 2 * b[t * width:(t + 1) * width], N) for t in range(terms))


def hamming_probe_long(bits, width, terms, secret, compressed=False, seed=None):
    """The client's probe for match_by_inner_long: (the TGSW words of the `terms` polynomials sum_i (1 - 2 b_i) X^(-i), one per
    chunk of `width` bits, as ONE selector record -- plain words for api.Selector, or with compressed=True one
    seed-compressed record for api.Selector.from_compressed --, and a CiphertextArray of ONE sample that encrypts (sum_i b_i)
    Delta over all terms * width bits, Delta = 2^-(log2(terms width) + 2)).  seed: the reproducible TGSW form."""
    params = secret.params
    _long_inner_shape(params, width, terms)
    polys = hamming_probe_long_polys(bits, width, terms, params.N)
    encrypt = api.tgsw_encrypt_polys_compressed if compressed else api.tgsw_encrypt_polys
    words = encrypt(polys, secret, seed=seed)
    addend = api.CiphertextArray(params, 1)
    api.encrypt_torus(addend.at(0), int((np.asarray(bits, dtype=np.int64).reshape(-1) & 1).sum()) * inner_delta(terms * width), secret)
    return words, addend


def match_by_inner_long(selector, gallery, terms, M, width, addend, tau, key, sample=0):
    """match_by_inner for entries of terms * width bits: `selector` holds hamming_probe_long's `terms` samples from `sample`
    on, `gallery` is pack_gallery_inner_long's groups (host words, or an int32 torch tensor resident on the device).
    api.ring_inner_sum -- ONE product launch, one key switch per entry --, then the unchanged decision tail with Delta =
    2^-(log2(terms width) + 2) and the addend sample.  TRUE iff distance <= tau; NOT exact within
    inner_sum_decision_band(params, inner_delta(terms * width), terms) of the threshold -- and that band (185 bits at P128 for
    2,048-bit codes) holds for probe codes whose bits look random.  The server cannot see the probe; a CLIENT whose code is
    all 0, all 1 or has long runs has s_i of one sign, a rounding weight up to N^3 / 12 a polynomial instead of (1 + N) w, and
    must take the band from inner_sum_decision_band(..., rounding_weight=hamming_probe_rounding_weight(bits, width, terms, N)):
    206 bits at P128 for an all-zero 2,048-bit code."""
    params = selector.params
    inner = api.CiphertextArray(params, M)
    api.ring_inner_sum(selector, sample, terms, gallery, M, width, key, inner, device=hasattr(gallery, "data_ptr"))
    return _hamming_decision(params, inner, M, terms * width, addend, tau, key)


def _masked_inner_shape(params, length, width, num, den):
    """_masked_shape under the term cap of this parameter set's gadget (api.inner_sum_max_terms)"""
    return _masked_shape(length, width, params.N, num, den, max_terms=api.inner_sum_max_terms(params))


def masked_gallery_inner(codes, masks, width, num, den, secret, seed=None):
    """Enrolment for match_by_inner_masked, the threshold's weights in the gallery's MESSAGES: M entries of L = chunks * width
    code bits g and mask bits n (1 = valid), sigma = 1 - 2 g.  Entry i of group i / S (S = N / width) takes, per chunk c, the
    TWO ring samples (i / S) terms + 2 c and + 2 c + 1, terms = 2 chunks, encrypting -den sigma_j n_j Delta and
    (den - 2 num) n_j Delta at coefficients (i mod S) width + j, Delta = masked_delta(den, L); centred for the decomposition.
    Returns int32 [R terms][(k+1) N]."""
    params = secret.params
    codes, masks = np.asarray(codes, dtype=np.int64) & 1, np.asarray(masks, dtype=np.int64) & 1
    if codes.ndim != 2 or codes.shape != masks.shape:
        raise ValueError("codes and masks are [M][L] bits of one shape")
    S, chunks = _masked_inner_shape(params, codes.shape[1], width, num, den)
    terms, delta = 2 * chunks, masked_delta(den, codes.shape[1])
    R = max(-(-len(codes) // S), 1)
    mu = np.zeros((R * terms, params.N), dtype=np.int64)
    for i in range(len(codes)):
        sig_n, n = (1 - 2 * codes[i]) * masks[i], masks[i]
        for c in range(chunks):
            at = slice((i % S) * width, (i % S + 1) * width)
            mu[(i // S) * terms + 2 * c, at] = -den * sig_n[c * width:(c + 1) * width] * delta
            mu[(i // S) * terms + 2 * c + 1, at] = (den - 2 * num) * n[c * width:(c + 1) * width] * delta
    return _encrypt_groups(mu, secret, seed)


def masked_probe_polys(bits, mask, width, N):
    """the 2 chunks probe polynomials of masked_probe_tgsw: per chunk s_i m_i and m_i in probe layout (0 / +-1) -> int32 [2 chunks][N]"""
    b, m = (np.asarray(x, dtype=np.int64).reshape(-1) & 1 for x in (bits, mask))
    if len(b) != len(m) or len(b) % width:
        raise ValueError("code and mask carry the same number of bits, whole chunks of %d" % width)
    polys = []
    for c in range(len(b) // width):
        at = slice(c * width, (c + 1) * width)
        polys += [probe_layout((1 - 2 * b[at]) * m[at], N), probe_layout(m[at], N)]
    return np.stack(polys).astype(np.int32)


def masked_probe_tgsw(bits, mask, width, num, den, secret, compressed=False, seed=None):
    """The client's probe for match_by_inner_masked: per chunk of `width` bits the TGSW samples of the TWO 0 / +-1
    polynomials s_i m_i and m_i in probe layout (s = 1 - 2 b, m the mask, 1 = valid), as ONE selector record of 2 chunks
    samples (plain, or seed-compressed).  The amplitude and the weights are the gallery's; there is no addend sample."""
    params = secret.params
    _masked_inner_shape(params, len(np.asarray(bits).reshape(-1)), width, num, den)
    encrypt = api.tgsw_encrypt_polys_compressed if compressed else api.tgsw_encrypt_polys
    return encrypt(masked_probe_polys(bits, mask, width, params.N), secret, seed=seed)


def probe_rounding_weight(values, N):
    """What the rounding errors of a centred ring sample are multiplied by in a coefficient of p c, p = sum_i v_i X^(-i) the
    probe polynomial of `values`: E_S[|p|_2^2 + |p S|_2^2] over a uniform binary ring key S (k = 1).  Coefficient j of p S is
    sum_i +-v_i S[j + i], the sign flipping past the wrap, so E (p S)[j]^2 = |v|^2 / 4 + sigma_j^2 / 4 with sigma_j = sum_(i <
    N - j) v_i - sum_(i >= N - j) v_i:  weight = |v|^2 (1 + N / 4) + sum_j sigma_j^2 / 4.  For coefficients of random signs
    sigma_j^2 ~ |v|^2 and the weight is (1 + N / 2) |v|^2, inside the header's (1 + N) |v|^2; for coefficients of ONE sign --
    the mask polynomial m of a masked probe -- sigma_j grows to |v|_1 and the weight to N^3 / 12 at N valid bits: 87 N |v|^2."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if not 1 <= len(v) <= N:
        raise ValueError("a probe carries 1..%d coefficients" % N)
    head = np.concatenate([[0.0], np.cumsum(v)])                  # head[c] = v_0 + .. + v_(c-1)
    first = head[np.minimum(N - np.arange(N), len(v))]            # the coefficients that do not wrap at j
    sigma = 2.0 * first - head[-1]
    n2 = float((v * v).sum())
    return n2 * (1.0 + N / 4.0) + float((sigma * sigma).sum()) / 4.0


def masked_rounding_weight(width, chunks, N):
    """the largest rounding weight of a masked probe of `chunks` chunks: per chunk a polynomial s m of random signs, held to
    the header's (1 + N) width, and a mask polynomial m with every bit valid, probe_rounding_weight of `width` ones"""
    return chunks * ((1.0 + N) * width + probe_rounding_weight(np.ones(width), N))


def inner_sum_product_variance(params, terms, norm2=None, ring_variance=None, rounding_weight=None):
    """COMPUTED variance of a coefficient of sum_t G_t (.) c_t before the key switch (torus units), the header's three terms
    summed over `terms` terms with (Bg/2)^2 for E[dig^2]: terms (k+1) l N (Bg/2)^2 bk^2 + W eps^2 / 3 + P v, P the probe's
    sum_t |p_t|_2^2 (default terms N, the most 0 / +-1 polynomials have), eps = 2^-(l Bgbit + 1) on a centred gallery, v the
    ring samples' variance (default bk^2, fresh ones), W the rounding weight: (1 + k N) P for probe coefficients of random
    signs (the default), sum_t probe_rounding_weight(p_t) in general -- far more for polynomials of one sign."""
    tl = params.ptr.contents.tgsw_params.contents.tlwe_params.contents
    bk = tl.alpha_min
    N, k, l = params.N, params.k, params.l
    P = terms * N if norm2 is None else norm2
    v = bk ** 2 if ring_variance is None else ring_variance
    W = (1 + k * N) * P if rounding_weight is None else rounding_weight
    eps = 2.0 ** -(l * params.Bgbit + 1)
    return terms * (k + 1) * l * N * (2.0 ** (params.Bgbit - 1)) ** 2 * bk ** 2 + W * eps ** 2 / 3.0 + P * v


def inner_sum_decision_band(params, delta, terms, rounding_weight=None):
    """clear_decision_band with the summed product's own noise in it: the smallest integer g with (g - 1/2) Delta >= 6 sigma,
    sigma^2 = inner_decision_sigma^2 + inner_sum_product_variance(params, terms, rounding_weight=...) (probe polynomials of
    norm^2 N, the largest), `delta` the torus word of Delta.  The decision of a match whose phase is (1/2 - D) Delta is
    guaranteed only where |D| >= g, and is NOT exact inside the band.  rounding_weight: None for probe coefficients of random
    signs (long templates), masked_rounding_weight for the masked route, whose mask polynomials have one sign.  COMPUTED at
    P128: 185 for long 2,048-bit codes (Delta = 2^-13, terms = 2); 6,571 in units of D (132 disagreeing bits at full validity) for masked 2,048-bit codes
    at 8/25 (Delta = 2^-18, terms = 4, masked_rounding_weight(1024, 2, 1024))."""
    d = int(delta) / 2.0 ** 32
    if d <= 0:
        raise ValueError("Delta must be positive")
    six = 6.0 * (inner_decision_sigma(params) ** 2 + inner_sum_product_variance(params, terms, rounding_weight=rounding_weight)) ** 0.5
    g = max(int(six / d + 0.5) - 1, 1)
    while (g - 0.5) * d < six:
        g += 1
    return g


def masked_inner_band(params, length, width, den):
    """inner_sum_decision_band of the masked route for entries of `length` bits in chunks of `width`"""
    chunks = length // width
    return inner_sum_decision_band(params, masked_delta(den, length), 2 * chunks, masked_rounding_weight(width, chunks, params.N))


def match_by_inner_masked(selector, gallery, M, width, length, num, den, key, sample=0):
    """Masked Hamming 1-to-N at the fractional threshold num / den against an ENCRYPTED gallery: `selector` holds
    masked_probe_tgsw's 2 L / width samples from `sample` on, `gallery` is masked_gallery_inner's groups (host words, or an
    int32 torch tensor resident on the device).  api.ring_inner_sum gives D Delta per entry -- ONE row, one key switch --;
    then Delta / 2 - D Delta (api.linear, a constant alone, recorded: no addend sample), the LUT bootstrap with the constant
    1/8 and one flush.  The weights are in the gallery's messages, so they are applied BEFORE the key switch, whose noise
    enters once (masked_weight_gain), and they do not enter the product's noise.  TRUE iff disagree / valid <= num / den --
    NOT exact where |D| < masked_inner_band(params, length, width, den)."""
    params = selector.params
    _, chunks = _masked_inner_shape(params, length, width, num, den)
    delta = masked_delta(den, length)
    inner = api.CiphertextArray(params, M)
    api.ring_inner_sum(selector, sample, 2 * chunks, gallery, M, width, key, inner, device=hasattr(gallery, "data_ptr"))
    return _masked_decision_tail(params, inner, M, delta, key)          # (its flush: the device form's gallery has been read)
