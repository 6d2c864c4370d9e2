"""The placement rule of the engine's pinned staging area (peba1_amd/csrc/host_stage.hpp), no GPU: where a reservation
goes, when the area's event is waited for first and when the area grows, through tfhe_hip_test_stage_place.  The cases
worked by hand, and a replay of seeded random request sizes against a restatement of the rule in which no two
reservations made since the last wait overlap."""
import ctypes as C
import functools

import numpy as np

ALIGN, START = 16, 256 << 10


@functools.lru_cache(maxsize=None)
def lib():
    from peba1_amd import lib as L
    return L.load()


def place(pos, capacity, outstanding, nbytes):
    """(offset, wait, capacity afterwards, write position afterwards)"""
    out = (C.c_int64 * 4)()
    assert lib().tfhe_hip_test_stage_place(pos, capacity, int(outstanding), nbytes, out) == 0
    return out[0], bool(out[1]), out[2], out[3]


def up(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def model(pos, capacity, outstanding, nbytes):
    """the rule restated: bump-allocate; what does not fit starts again at 0 behind the outstanding uploads, in an area
    that grows to half again the request (never below its starting size) when the request is larger than it"""
    at, need = up(pos), up(nbytes)
    if at + need <= capacity:
        return at, False, capacity, at + need
    if need > capacity:
        capacity = max(START, up(need + need // 2))
    return 0, bool(outstanding), capacity, need


def test_first_request_on_an_empty_area():
    assert place(0, 0, False, 100) == (0, False, START, 112)          # nothing allocated yet: the starting size, no wait
    assert place(0, START, False, 100) == (0, False, START, 112)
    assert place(0, START, True, 4) == (0, False, START, 16)


def test_exact_fit_and_one_byte_more():
    pos = START - 4096
    assert place(pos, START, True, 4096) == (pos, False, START, START)           # exactly the remainder
    assert place(pos, START, True, 4097) == (0, True, START, 4112)               # an upload outstanding: wait, offset 0
    assert place(pos, START, False, 4097) == (0, False, START, 4112)             # nothing outstanding: no wait, offset 0
    assert place(START, START, True, 1) == (0, True, START, 16)                  # a full area


def test_a_request_larger_than_the_area_makes_it_grow():
    for outstanding in (False, True):
        for pos in (0, 4096, START):
            off, wait, cap, nxt = place(pos, START, outstanding, START + 1)
            assert off == 0 and wait == outstanding and nxt == up(START + 1)
            assert cap >= (START + 1) + (START + 1) // 2 and cap % ALIGN == 0
    # a small request on an area that holds nothing yet still gets the starting size; one that fits does not grow it
    assert place(0, 0, False, 1)[2] == START and place(16, START, True, START - 16)[2] == START
    assert place(0, 3 * START, True, 2 * START) == (0, False, 3 * START, 2 * START)


def test_offsets_are_aligned_whatever_the_position():
    for pos in (0, 1, 15, 16, 17, 1000, START - 17):
        for nbytes in (0, 1, 4, 15, 16, 17, 4000):
            off, wait, cap, nxt = place(pos, START, True, nbytes)
            assert off % ALIGN == 0 and nxt % ALIGN == 0 and off + nbytes <= nxt <= cap, (pos, nbytes)
            assert (off, wait, cap, nxt) == model(pos, START, True, nbytes)


def test_bad_arguments_are_refused():
    out = (C.c_int64 * 4)()
    assert lib().tfhe_hip_test_stage_place(-1, START, 0, 4, out) == -1
    assert lib().tfhe_hip_test_stage_place(0, START, 0, -4, out) == -1
    assert lib().tfhe_hip_test_stage_place(0, START, 0, 4, None) == -1
    lib().tfhe_hip_clear_error()


def test_random_replay_against_the_model_never_overlaps_live_reservations():
    """4,000 requests -- mostly slot lists of a few words to a few thousand, now and then one larger than the area -- each
    followed by its upload; now and then the stream is synchronised (the area goes idle).  The entry agrees with the model
    at every step, and no reservation overlaps another made since the last wait, synchronisation or reallocation"""
    rng = np.random.default_rng(0x57A6E)
    pos, capacity, outstanding, live = 0, 0, False, []
    waits = grows = wraps = 0
    for step in range(4000):
        kind = rng.integers(0, 100)
        nbytes = int(rng.integers(0, 64) if kind < 10 else rng.integers(1, 70000))
        if kind >= 98 and capacity < 2 * START:
            nbytes = int(rng.integers(1, 4)) * capacity + 1
        got = place(pos, capacity, outstanding, nbytes)
        assert got == model(pos, capacity, outstanding, nbytes), (step, pos, capacity, outstanding, nbytes)
        off, wait, new_capacity, nxt = got
        assert off % ALIGN == 0 and off + nbytes <= new_capacity and nxt == off + up(nbytes)
        if new_capacity != capacity:
            assert new_capacity >= nbytes + nbytes // 2
            grows += 1
        if off == 0 and pos > 0:
            # from the start again: what was reserved before may only be reused behind a wait, or when nothing was outstanding
            assert wait == outstanding
            wraps += 1
            live = []
        waits += wait
        for a, b in live:
            assert off >= b or off + nbytes <= a, (step, (off, nbytes), (a, b))
        live.append((off, off + nbytes))
        pos, capacity, outstanding = nxt, new_capacity, True         # uploaded()
        if rng.integers(0, 8) == 0:
            outstanding = False                                      # the stream was synchronised: idle, the position stays
    assert waits > 50 and grows >= 2 and wraps > waits + 5, (waits, grows, wraps)   # every path, wraps without a wait included
