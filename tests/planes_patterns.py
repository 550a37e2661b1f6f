"""What tests/test_present_planes.py and tests/test_present_planes_cpu.py share: the film sizes of the layout cases, planes full of distinct
word patterns (with the words a copy must not touch: NaN payloads, -0.0, denormals, infinities, 0xFFFFFFFF), sentinel planes, the plane sets."""
import numpy as np

# (width, height, world): ragged in both axes (10 x 6 tiles); another ragged one; narrower than a tile (ranks 1 .. 3 own nothing); one tile
LAYOUT_CASES = [(76, 44, 1), (76, 44, 2), (76, 44, 3), (76, 44, 8), (61, 37, 3), (7, 5, 4), (8, 8, 4)]
# distributed.PLANE_ORDER's keys with their trailing shape and dtype as the library's readers return them
PLANES = [("film", (3,), np.float32), ("albedo", (3,), np.float32), ("normal", (3,), np.float32), ("emission", (3,), np.float32),
          ("depth", (), np.float32), ("alpha", (), np.float32), ("id", (2,), np.uint32), ("moments", (3,), np.float32),
          ("history", (), np.float32), ("counts", (), np.float32), ("motion", (4,), np.float32)]
SINGLE_BITS = [1, 2, 4, 8, 16, 32]
MIXED = 1 | 4 | 32          # C, M and Q: the first plane, one from the middle, the four-channel one
PLANE_SETS = [63] + SINGLE_BITS + [MIXED]
SPECIAL_WORDS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0xFFFFFFFF, 0x00000000], np.uint32)
SENTINEL = 0xA5A5A5A5


def make_planes(w, h, seed=1):
    """-> {key: array [h, w] + tail}: every word of every plane distinct from its neighbours and from the other planes' (plane number in the
    top bits, word index below), the film uniform in [-0.5, 1.5) so that the bgra8 rule meets all its branches, and the special words sown
    into every plane at seeded places (the first and the last word among them)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, (key, tail, dtype) in enumerate(PLANES):
        n = w * h * int(np.prod(tail, dtype=np.int64))
        if key == "film":
            words = rng.uniform(-0.5, 1.5, n).astype(np.float32).view(np.uint32).copy()
        else:
            words = (np.uint32((k + 1) << 26) | np.arange(n, dtype=np.uint32))
        where = np.concatenate([[0, n - 1], rng.integers(0, n, 2 * len(SPECIAL_WORDS) - 2)])
        words[where] = np.tile(SPECIAL_WORDS, 2)
        out[key] = words.view(dtype).reshape((h, w) + tail)
    return out


def sentinel_planes(w, h):
    out = {key: np.full((h, w) + tail, SENTINEL, np.uint32).view(dtype) for key, tail, dtype in PLANES}
    out["bgra8"] = np.full((h, w, 4), 0xA5, np.uint8)
    return out


def same_words(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()
