"""The identities the compact walk's cut keys rest on (csrc/extend_kernel.h: pop_cut, push_cut, entry_within, LaneStack::BOTTOM), on bit patterns.

A stack entry is (bits(a) & 0xFFFFC000) | w: the entry distance a >= +0 truncated to its top 18 bits over a 14-bit child word.  The kernels
compare the RAW entry, as an unsigned integer, with a key made of the best hit's distance b; these tests say that this is the float compare it
replaced, for every pair of the values where the two could part: zero, denormals, neighbours, values that differ only below the truncation,
FLT_MAX and +inf.  The constants are read from the sources, so a change there is checked, not a copy of it.
"""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-file-vulkan-pathtracing_amd", "csrc")
KEY_MASK, WORD_MASK = np.uint32(0xFFFFC000), np.uint32(0x3FFF)
INF_BITS, FLT_MAX_BITS = 0x7F800000, 0x7F7FFFFF


def _source_constants():
    ek = open(os.path.join(CSRC, "extend_kernel.h")).read()
    ls = open(os.path.join(CSRC, "lds_scene.h")).read()
    done = int(re.search(r"C14_DONE = (0x[0-9A-Fa-f]+)u", ls).group(1), 16)
    bottom_key = int(re.search(r"BOTTOM = (0x[0-9A-Fa-f]+)u \| C14_DONE;", ek).group(1), 16)
    pop_or = int(re.search(r"pop_cut\(float best_t\) \{ return __float_as_uint\(best_t\) \| (0x[0-9A-Fa-f]+)u; \}", ek).group(1), 16)
    cap = int(re.search(r"push_cut\(float best_t\) \{ return min\(pop_cut\(best_t\), (0x[0-9A-Fa-f]+)u\); \}", ek).group(1), 16)
    assert re.search(r"entry_within\(uint32_t e, uint32_t cut\) \{ return e <= cut; \}", ek)
    return done, bottom_key | done, pop_or, cap


DONE, BOTTOM, POP_OR, PUSH_CAP = _source_constants()


def pop_cut(b_bits):
    return b_bits | np.uint32(POP_OR)


def push_cut(b_bits):
    return np.minimum(pop_cut(b_bits), np.uint32(PUSH_CAP))


def distances():
    """bit patterns of non-negative floats: random ones over the whole range, and the places where an integer and a float compare could differ"""
    rng = np.random.default_rng(2024)
    rnd = rng.integers(0, INF_BITS, 600, dtype=np.uint32)                              # any exponent, denormals included
    unit = rng.uniform(0.001, 10000.0, 200).astype(np.float32).view(np.uint32)         # the distances a render sees
    base = np.concatenate([rnd[:60], unit[:40]])
    special = [0x00000000, 0x00000001, 0x00000002, 0x007FFFFF, 0x00800000,            # +0, the smallest denormals, the largest, the smallest normal
               0x00003FFF, 0x00004000, 0x3F800000, FLT_MAX_BITS - 1, FLT_MAX_BITS, INF_BITS]
    near = [base - 1, base + 1]                                                        # one ulp apart
    same18 = [(base & KEY_MASK), (base & KEY_MASK) | WORD_MASK, (base & KEY_MASK) | np.uint32(0x2000)]   # equal in their top 18 bits
    next18 = [(base & KEY_MASK) + np.uint32(0x4000), (base & KEY_MASK) - np.uint32(1)]  # ... and the neighbours of that range
    v = np.concatenate([rnd, unit, np.uint32(special), *near, *same18, *next18]).astype(np.uint32)
    v = np.unique(v[v <= INF_BITS])
    assert v[0] == 0 and v[-1] == INF_BITS
    return v


def words(n):
    rng = np.random.default_rng(7)
    return [np.zeros(n, np.uint32), np.full(n, 0x3FFF, np.uint32), rng.integers(0, 0x4000, n, dtype=np.uint32)]


def test_source_constants():
    assert POP_OR == 0x3FFF and PUSH_CAP == FLT_MAX_BITS and DONE == 0x3FFF
    assert BOTTOM == DONE      # key +0


def test_raw_entry_compare_is_the_float_compare():
    """identity 1: entry <= bits(b) | 0x3FFF  <=>  !(float(entry & 0xFFFFC000) > b), all pairs, all child words"""
    v = distances()
    b_bits = v[None, :]
    b = v.view(np.float32)[None, :]
    for w in words(len(v)):
        entry = ((v & KEY_MASK) | w)[:, None]
        as_int = entry <= pop_cut(b_bits)
        with np.errstate(invalid="ignore"):
            as_float = ~((entry & KEY_MASK).view(np.float32) > b)
        assert as_int.shape == (len(v), len(v)) and (as_int == as_float).all(), np.argwhere(as_int != as_float)[:4]
    # (both outcomes occur, so the comparison above is about something)
    assert as_int.any() and not as_int.all()


def test_the_cull_keeps_equal_distances():
    """the cull is <=: an entry whose distance IS the best hit's survives (the lowest-primitive-id rule needs the candidate)"""
    v = distances()
    for w in words(len(v)):
        entry = (v & KEY_MASK) | w
        assert (entry <= pop_cut(v)).all()
        fin = v < INF_BITS
        assert (entry[fin] <= push_cut(v[fin])).all()


def test_stacked_entries_see_one_cut():
    """an entry that was pushed (its key is within the cap) gives the same verdict against push_cut and pop_cut: a node step uses its push cut
    for the pop that follows it"""
    v = distances()
    for w in words(len(v)):
        entry = ((v & KEY_MASK) | w)[:, None]
        stacked = entry <= np.uint32(PUSH_CAP)
        same = (entry <= pop_cut(v[None, :])) == (entry <= push_cut(v[None, :]))
        assert same[np.broadcast_to(stacked, same.shape)].all()


def test_bottom_is_within_every_cut():
    """identity 2: the BOTTOM entry is taken by every pop, whatever the best hit"""
    v = distances()
    assert (np.uint32(BOTTOM) <= push_cut(v)).all() and (np.uint32(BOTTOM) <= pop_cut(v)).all()
    assert BOTTOM & 0x3FFF == DONE


def test_no_miss_key_passes_the_push_cut():
    """identity 3: +inf | w is above min(bits(b) | 0x3FFF, FLT_MAX bits) for every b, +inf included: no miss is pushed or entered"""
    v = distances()
    for w in words(len(v)):
        miss = (np.uint32(INF_BITS) | w)[:, None]
        assert not (miss <= push_cut(v[None, :])).any()
    assert (push_cut(np.uint32([INF_BITS])) == FLT_MAX_BITS).all()
    # ... and every finite key is within it when nothing was hit yet and tmax is +inf
    assert (((v[v < INF_BITS] & KEY_MASK) | WORD_MASK) <= push_cut(np.uint32([INF_BITS]))).all()


def test_keys_order_like_their_distances():
    """a child behind the cut sorts behind every child within it: keys compare like the truncated distances, then like the words"""
    v = distances()
    rng = np.random.default_rng(3)
    a, c = rng.choice(v, 4000), rng.choice(v, 4000)
    wa, wc = rng.integers(0, 0x4000, 4000, dtype=np.uint32), rng.integers(0, 0x4000, 4000, dtype=np.uint32)
    ka, kc = (a & KEY_MASK) | wa, (c & KEY_MASK) | wc
    ta, tc = (a & KEY_MASK).view(np.float32), (c & KEY_MASK).view(np.float32)
    lt = ta < tc
    assert lt.any() and (ka[lt] < kc[lt]).all()
