"""The host side of the matrix key switch (ks_matrix.hpp, launch_plan.hpp): the signed byte planes of a key word and the
planner's new form, without a GPU.

The byte planes are what makes the int8 product exact: sum_p s_p 2^(8p) = w (mod 2^32) with every s_p in [-128, 127].  The
planner gives the matrix form to a flush's launch at and above ks_matrix_min where a tiled form would have run and the key
holds its image; the entries without a word for the new tunings return what they always did."""
import ctypes as C

import numpy as np

import ks_common as K

CORNERS = [0, 0x80, 0x7F, 0x80808080, 0x7F7F7F7F, 0xFFFFFFFF, 0x80000000]
MATRIX = 3
P128 = (630, 1024, 1, 8, 2)


def planes(words):
    from peba1_amd import lib
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros((len(w), 4), dtype=np.int8)
    rc = lib.load().tfhe_hip_test_ks_byte_planes(w.ctypes.data_as(C.POINTER(C.c_uint32)), len(w),
                                                 out.ctypes.data_as(C.POINTER(C.c_int8)))
    assert rc == 0
    return out


def test_byte_planes_sum_to_the_word():
    rng = np.random.default_rng(0x4B5)
    words = np.concatenate([np.array(CORNERS, dtype=np.uint32), rng.integers(0, 2 ** 32, 10 ** 5, dtype=np.uint32)])
    s = planes(words).astype(np.int64)
    assert s.min() >= -128 and s.max() <= 127
    back = (s * (256 ** np.arange(4, dtype=np.int64))[None, :]).sum(axis=1) % 2 ** 32
    bad = np.flatnonzero(back != words.astype(np.int64))
    assert bad.size == 0, (bad[:4], words[bad[:4]], s[bad[:4]])
    # the corners, written out: a byte of 128 or more becomes negative and carries
    assert s[:7].tolist() == [[0, 0, 0, 0], [-128, 1, 0, 0], [127, 0, 0, 0], [-128, -127, -127, -127], [127, 127, 127, 127],
                              [-1, 0, 0, 0], [0, 0, 0, -128]]


def plan2(shape, tunings, has_image, cu, count):
    from peba1_amd import lib
    tn = {**K.KS_DEFAULTS, "ks_matrix": 1, "ks_matrix_min": 512, **tunings}
    t7 = (C.c_int32 * 7)(*([tn[k] for k in K.KS_DEFAULTS] + [tn["ks_matrix"], tn["ks_matrix_min"]]))
    out = (C.c_int64 * 7)()
    assert lib.load().tfhe_hip_test_ks_plan_form2(*shape, t7, has_image, cu, count, out) == 0
    return tuple(out)


def plan_old(shape, tunings, cu, count):
    from peba1_amd import lib
    n, N, k, t, bb = shape
    assert k == 1
    return K.ks_plan(lib.load(), n, t, bb, tunings, cu, count, N=N)


def test_entries_without_the_new_tunings_return_the_form_off():
    """what they returned before this form existed: never form 3, whatever the width; at P128 the index form, 16 gates"""
    for count in (1, 31, 32, 511, 512, 513, 2048, 8192, 8193, 20000):
        for tunings in ({}, {"ks_tile": 24}, {"ks_index": 0}, {"ks_tile": 0}):
            old = plan_old(P128, tunings, 256, count)
            assert old[6] in (K.PERGATE, K.STRIP, K.INDEX)
            assert plan2(P128, dict(tunings, ks_matrix=0), 1, 256, count) == old
    assert plan_old(P128, {}, 256, 4096)[:3] + plan_old(P128, {}, 256, 4096)[6:] == (1, 16, 8192, K.INDEX)


def test_form2_gives_the_matrix_form_at_and_above_the_threshold():
    for least in (64, 128, 512, 2048):
        for count in (1, 32, least - 1, least, least + 1, 4 * least, 8192 + 5):
            got = plan2(P128, {"ks_matrix_min": least}, 1, 256, count)
            if count >= least:
                assert got == (1, 64, count, 1, 1, 0, MATRIX), (least, count, got)
            else:
                assert got == plan_old(P128, {}, 256, count), (least, count, got)
    # only where a tiled form would have run: not the per-gate kernel's widths and decompositions, not ks_tile 0
    assert plan2((1023, 1024, 1, 8, 2), {}, 1, 256, 4096)[6] == K.PERGATE          # 256 threads a row
    assert plan2((630, 1024, 1, 4, 4), {}, 1, 256, 4096)[6] == K.PERGATE
    assert plan2(P128, {"ks_tile": 0}, 1, 256, 4096)[6] == K.PERGATE
    assert plan2(P128, {"ks_index": 0}, 1, 256, 4096)[6] == MATRIX
    assert plan2((500, 1024, 1, 8, 2), {}, 1, 256, 4096)[6] == MATRIX
    assert plan2((1024, 2048, 1, 8, 2), {}, 1, 256, 4096)[6] == MATRIX


def test_a_key_without_its_image_plans_the_old_form():
    for count in (512, 4096, 8193):
        for tunings in ({}, {"ks_matrix_min": 64}, {"ks_index": 0}):
            assert plan2(P128, tunings, 0, 256, count) == plan_old(P128, {k: v for k, v in tunings.items() if k in K.KS_DEFAULTS},
                                                                   256, count)
