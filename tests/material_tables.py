"""Material tables and environments at the edges of the value range, and the rule by which a film rendered from them is compared
with the oracle's.  Plain numpy, no test machinery: tests/test_material_edges.py and scripts/fuzz_render.py --materials share it."""
import numpy as np

f32, u32 = np.float32, np.uint32
INF = float("inf")

KD_EDGE = f32([0.0, -0.0, 1e-45, -3e-42, 2.0 ** -101, 2.0 ** -100, 2.0 ** -99, 2.0 ** -97, -2.0 ** -98, 0.3, 0.8, 1.0, -0.6, 7.0])
KE_EDGE = f32([0.0, -0.0, 1e-45, -2e-40, 5.0, -3.0, 0.25])
KD_HUGE = f32([2.0 ** 118, 2.0 ** 121, -2.0 ** 122, 3e38, 2.0 ** 60])
KE_HUGE = f32([3e38, -1e30, 1e30])
ENV_MIXED = (0.7, -0.6, 0.0)
ENV_TINY = (0.0, -0.0, 1e-44)
ENV_GUARD = (0.7, -0.6, 0.25)        # every channel shows its weights (the guard table)
ENV_HUGE = (3e38, 1e-45, -1e30)      # finite; overflows at the second sample's add
ENV_INF = (INF, 0.5, -INF)           # the cull stands down for it (render.hip apply_cull)
# the box pushed to the right edge of the image (a view of test_fused_subject_first_order_changes_no_bit): culled pixels carry `env`
SIDE_CAM = dict(cam_origin=(1.1, -1.0, 5.0), cam_target=(1.1, -1.0, 2.0))
GUARD_LO, GUARD_HI = f32(2.0 ** -100), f32(2.0 ** 120)     # ptm::div3_by_pdf's guard (pt_math.h)


# ---- material tables ------------------------------------------------------------------------------------------------------------
def table_a(n, seed, all_emit=False):
    """Family A, "no overflow possible": -> float32 [n, 6] {Kd, Ke}.  Kd channels drawn independently from KD_EDGE, Ke channels from
    KE_EDGE for about 35 % of the triangles (all of them with all_emit; the others +0); about two thirds of the triangles get one
    Kd channel reset to uniform(0.3, 1) so that paths keep carrying visible weight."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 6), f32)
    t[:, :3] = KD_EDGE[rng.integers(0, len(KD_EDGE), (n, 3))]
    ke = KE_EDGE[rng.integers(0, len(KE_EDGE), (n, 3))]
    emits = np.ones(n, bool) if all_emit else rng.random(n) < 0.35
    t[emits, 3:] = ke[emits]
    reset, ch, val = rng.random(n) < 2.0 / 3.0, rng.integers(0, 3, n), rng.uniform(0.3, 1.0, n).astype(f32)
    t[np.nonzero(reset)[0], ch[reset]] = val[reset]
    return t


def table_b(n, seed):
    """Family B, "overflow": table_a(n, seed) with about one triangle in nine given Kd channels from KD_HUGE and about one in eighteen
    Ke = KE_HUGE."""
    t = table_a(n, seed)
    rng = np.random.default_rng(seed + 7919)
    big = rng.random(n) < 1.0 / 9.0
    t[big, :3] = KD_HUGE[rng.integers(0, len(KD_HUGE), (n, 3))][big]
    t[rng.random(n) < 1.0 / 18.0, 3:] = KE_HUGE
    return t


def table_g(n, seed):
    """The guard table, beyond the issue's families: Kd channels are, half of them, +-2^-k with k in 112 .. 128, the others uniform(0.3, 1);
    no emitters.  Family A's values around 2^-100 put the dividend x = (Kd / pi) * cos on both sides of div3_by_pdf's guard, but just below
    it the short quotient is still almost always the correctly rounded one: its residual loses bits only once it turns denormal, and a
    wrong rounding needs a dividend well below 2^-100 (a few in a million cosines at Kd = 2^-102 and 2^-104, where only small cosines
    take x that low).  Restated on the CPU with fmaf, the three-instruction sequence differs from x / pdf for 0.03 % of uniform cosines at
    Kd = 2^-112, 1 % at 2^-118, 17 % at 2^-124 and 3 % at 2^-128; never for a dividend inside the guard.  Under a visible env a pixel's channel whose first hits all have such a Kd holds
    nothing but these quotients' products, so one wrong rounding shows in the film."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 6), f32)
    tiny = np.ldexp(f32(1.0), -rng.integers(112, 129, (n, 3))).astype(f32) * np.where(rng.random((n, 3)) < 0.25, f32(-1), f32(1))
    t[:, :3] = np.where(rng.random((n, 3)) < 0.5, tiny, rng.uniform(0.3, 1.0, (n, 3)).astype(f32))
    return t



# ---- the comparison rule --------------------------------------------------------------------------------------------------------
def _bits(a, exact):
    b = np.ascontiguousarray(a, f32).view(u32).copy()
    if not exact:
        b[np.isnan(a)] = u32(0x7FC00000)
    return b


def assert_same(case, what, got, want, exact):
    """got == want, float32 arrays of one shape [H, W, C].  exact (family A): the bytes are equal.  Otherwise (family B) the NaN
    positions are equal and every other value is bit-equal: a NaN that the arithmetic GENERATES (inf * 0, inf - inf) is 0xFFC00000 on
    x86, the oracle's machine, and 0x7FC00000 on the GPU, and which of two NaN operands an add passes on differs too, so both sides
    have every NaN replaced by one pattern before the bits are compared.  No NaN is an input.  A mismatch names the case, the pixel,
    the channel and both bit patterns."""
    assert got.dtype == f32 and want.dtype == f32 and got.shape == want.shape, (case, what, got.dtype, got.shape, want.shape)
    g, w = _bits(got, exact), _bits(want, exact)
    if g.tobytes() == w.tobytes():
        return
    bad = np.argwhere(g != w)
    y, x, ch = (int(k) for k in bad[0])
    raise AssertionError(f"{case}, {what}: {len(bad)} of {g.size} values differ; first at pixel ({x}, {y}) channel {ch}: "
                         f"got 0x{int(g[y, x, ch]):08x}, oracle 0x{int(w[y, x, ch]):08x}")
