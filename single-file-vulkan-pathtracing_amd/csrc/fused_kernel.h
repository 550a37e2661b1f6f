// fused_kernel.h -- PT_PIPELINE_FUSED: the radiance loop as ONE persistent kernel for scenes that live in LDS.
//
// The reference's raygen shader is itself a megakernel: one invocation owns its path state from the first sample of its
// pixel to the last (raygen.rgen:41-91), and traceRayEXT / the closest-hit and miss shaders run inside it.  The wavefront
// pipeline (render.hip, shade_kernels.hip) splits that into k_extend / k_shade over queues in HBM -- 150 B of queue traffic per ray and a
// workspace of tens of GB -- because big scenes need the sorting, the compaction and the long launches.  A scene of a few
// dozen triangles needs none of it: nodes, triangles and the shading tables fit LDS, so here a lane keeps its path from
// bounce to bounce and HBM sees the radiance of a slot only (16 B per slot, or 16 B per logged term with sample groups).
//
//   * traversal: the compact walk of extend_kernel.h (`extend_body<true, false, false, PAIRS>`; pair leaves: one-dword stack
//     entries in LDS, key-sorted children, fan pairs tested together), restated here operation for operation -- the hot
//     instantiation of that template is register-allocated to the last VGPR and must not grow a second use;
//   * a lane whose ray is finished WAITS with its hit in registers until `refill` / 64 of the wave's live lanes wait too
//     (36 / 64: fused.hip), then all of them run the shade block -- closesthit.rchit:50-65 / miss.rmiss:8-12, the bounce of
//     raygen.rgen:76-83, the next sample's camera ray (raygen.rgen:45-60), or the first sample of a NEW slot -- and set up
//     their next ray; the same operations on the same operands as k_shade, per lane in the same order, so the film is the wavefront pipeline's bit
//     for bit.  The steps a bounce and a camera ray share (two rand, one square root) run once for both kinds of lanes (step (3) below);
//   * slots (frame, sample group, pixel) are handed out in order by device-scope counters -- eight, one per XCD's share of the
//     workgroups, with work stealing between them -- PT_FUSED_BATCH at a time per wave, so a wave that drew cheap border
//     pixels simply takes more of them: no tail beyond the last batch's own length;
//   * path state that only the shade block touches (slot, sample | depth, seed, weight, pixel, the slot's colour or its
//     term count) lives in LDS, [field][thread]: the traversal loop keeps the registers it has in k_extend_lds7p;
//   * control flow is written for the CU's ONE scalar unit (round 6: it was as busy as the vector units -- DESIGN.md section 6): the loops inside
//     the persistent loop (node steps, pops) run on the WAVE's condition, with the lanes that are served behind one exec mask; no `continue`
//     (one way back to the loop's head); selects instead of short-circuit branches where the wave runs both sides anyway; no loop-carried
//     flag where a register says the same (`cur != DONE`); every kernel argument in a scalar register of its own (ptm::own_sgprs).  The shade
//     block's step (1) follows the same rule: a pass of ~45 lanes holds misses and surface hits, emitters and others, ended and continuing paths
//     all at once, so a miss is one more record of the shade table (no miss / surface split), one sample group adds its term without a vote
//     (adding +-0 keeps an accumulator's bits), and a path's end is selects -- only a complete slot, which stores, is a branch.
//
// Radiance goes where the wavefront pipeline puts it (struct Radiance): one accumulator per slot written when the slot is
// complete (one sample group), or the ordered term logs that k_resolve replays (several groups) -- k_resolve is shared.
#pragma once
#include "radiance_device_kernel.h"  // (RAYS: the index arithmetic of the hand-out and the seed rule, shared with the host's restatement test)

// Block shape: the scene tables (9.2 KB for the Cornell box) are per block, the stack and the path state (20 dwords) per
// thread, so bigger blocks leave more of the 160 KB to waves: 256 threads = 5 blocks = 5 waves per SIMD; 512 threads =
// 50.2 KB = 3 blocks = 6 waves per SIMD at 80 VGPRs (1 - 2 dwords spilled).  Same box, interleaved: 36.2 -> 38.1 Grays/s
// (profiles/r04d_ab_fused_tb.log); 4 waves: 31.4.  Round 6's kernel: 768 x 6 waves -1 %, 256 -7 %, 384 -14 % (profiles/r06q_fused_block_size.log).
#ifndef PT_FUSED_WAVES
#define PT_FUSED_WAVES 6
#endif

#ifndef PT_FUSED_TB
#define PT_FUSED_TB 512
#endif
constexpr int FTB = PT_FUSED_TB;

#ifndef PT_FUSED_BATCH
#define PT_FUSED_BATCH 256  // most slots a wave draws per atomic (a multiple of 64: 64 consecutive slots are one 8x8 tile)
#endif
// ... with one sample group: ONE tile.  A wave hands a batch to its lanes as they finish their slots, so the last slot of a batch STARTS
// (batch / 64 - 1) slot lengths after the batch was drawn -- with 256 and slots of 32 samples (1.5 - 2.6 ms each) interior slots drawn 6 ms
// before the counters ran dry were still being started after it, whatever the hand-out order (the wave timeline of
// scripts/probe_fused_timeline.py: profiles/r05b_fused_timeline.log -> r05c_fused_timeline64.log).  64 / 128 / 256, 1080p Cornell box, Grays/s:
// K = 16 41.2 / 41.4 / 40.8; K = 4 38.8 / 37.7 / 33.8; K = 2 36.0 / 32.6 / 27.3; a rank of world 8 at 16 frames 36.1 / 33.0 / 27.2
// (profiles/r05c_fused_batch1.log).  The guided self-scheduling the bigger batches needed at the end of a launch is gone with them.
#ifndef PT_FUSED_BATCH1
#define PT_FUSED_BATCH1 64
#endif
#define PT_FUSED_WTILES (PT_FUSED_BATCH / 64)  // tile words a wave keeps in LDS for its current batch
#define PT_FUSED_PARTS 8          // slot counters (one per XCD's share of the workgroups)
#define PT_FUSED_PART_STRIDE 32   // ... in dwords: one 128-B line each

// path state in LDS, [field][thread]
enum : int { FS_SLOT = 0, FS_CTR, FS_SEED, FS_WR, FS_WG, FS_WB, FS_PXY, FS_A, FS_B, FS_C, FS_MB, FS_FIELDS };
// FS_A..C: the slot's colour (one sample group) | FS_A: its term count (several groups)
// FS_MB: maxSamples * frame + 1 of the slot's frame (raygen.rgen:47: the seed's multiplier less the sample number), kept so that a
// sample's camera ray does not decode slot -> frame again (two divisions by run-time constants, at the ten lanes of that block)
// NEE (PT_FLAG_NEE, k_fused_nee): a shadow ray walks between a hit and its bounce.  What the lane needs across that walk, [field][thread] behind the
// waves' tile words (where the instrumented twin keeps its counters: NEE has no such twin):
//   FS_NEE_POS: PT_MISS while a path ray walks; while a shadow ray walks, the hit it left (its bounce is drawn when it returns)
//   FS_NEE_R..B: the light sample's contribution, added if the shadow ray reaches the light
// (the hit's position is the shadow ray's origin: read back from the permuted origin the walk keeps in registers)
enum : int { FS_NEE_POS = 0, FS_NEE_R, FS_NEE_G, FS_NEE_B, FS_NEE_FIELDS };
// waves per SIMD of the NEE instantiation: its four more dwords per thread leave room for two 512-thread blocks per CU (the Cornell box:
// ~60 KB each), so the compiler may use the registers of four waves
#ifndef PT_FUSED_WAVES_NEE
#define PT_FUSED_WAVES_NEE 4
#endif

// ---- the LDS plan, in bytes from LDS byte 0: fused.hip sizes the launch with it, the kernel takes its pointers from it.
// nodes | three permuted triangle copies | shade4, then the miss record | tangent frames || path state | the waves' tile words | stack (the BOTTOM entry's level, then
// level 0 ...: LaneStack) | extra
// The path state lies IN FRONT of the stack: LaneStack's `under`, one level below the BOTTOM entry, is an address inside it -- compared with, never
// read or written through -- so the stack costs no level of its own for it (one more 2-KB level is the third block per CU).
// The scene's tables come FIRST: the kernel has no static LDS, so they start at LDS address 0 and a node's address is its number times the
// stride -- no base register in the node step.  What a run-time count places (the stack, the state) is reached through per-lane pointers anyway.
// extra: the shadow ray's state (NEE) or the block counters (COUNT), never both.
struct FusedLds { uint32_t wide, tri, shade, frame, stack, state, wtile, extra; };
__host__ __device__ constexpr FusedLds fused_lds(uint32_t n_wide, uint32_t n_tris, uint32_t stack_levels)
{
    FusedLds l{};
    l.wide = 0u;
    l.tri = l.wide + (uint32_t)lds_nodes_bytes(n_wide);
    l.shade = l.tri + (uint32_t)lds_tris_bytes(n_tris);
    l.frame = l.shade + (uint32_t)sizeof(float4) * 3u * (n_tris + 1u);  // (record n_tris: the miss -- weight * env as the Ke of a hit that ends its path)
    l.state = l.frame + (uint32_t)sizeof(float4) * 2u * n_tris;
    l.wtile = l.state + (uint32_t)sizeof(uint32_t) * FS_FIELDS * FTB;
    l.stack = l.wtile + (uint32_t)sizeof(uint32_t) * (FTB / 64) * PT_FUSED_WTILES;
    l.extra = l.stack + (uint32_t)compact_stack_bytes(FTB, stack_levels);  // (its extra level is the BOTTOM entry's)
    return l;
}
constexpr int PT_FUSED_POP_N_MAX = 4;  // entries a pass of the pop loop may read together (PT_FUSED_POP_N below)
// pair_leaf_test<LOAD_D_FIRST> reads the record five float4 behind a leaf's first: for a single triangle at the last position of the last copy
// that is ptl::D_FIRST_OVERREAD_F4 float4 past the triangle copies -- the shade table must start right there and be at least that long
constexpr bool fused_lds_covers_leaf_read(uint32_t n_wide, uint32_t n_tris)
{
    const FusedLds l = fused_lds(n_wide, n_tris, 1u);
    // (... and PT_FUSED_POP_N_MAX stack levels and a dword of other LDS in front of the stack: the pop's reads of the levels under the BOTTOM
    // entry, PT_FUSED_POP_N_MAX - 1 at the most, stay inside the block's LDS, and `under` and a parked pointer, a level and a dword below
    // BOTTOM and held as many levels lower again (LaneStack's LOW), are no wrapped addresses)
    return l.shade == l.tri + lds_tris_bytes(n_tris) && l.frame - l.shade >= sizeof(float4) * ptl::D_FIRST_OVERREAD_F4 && l.wide == 0u &&
           l.stack >= l.state + sizeof(uint32_t) * FTB * PT_FUSED_POP_N_MAX + 4u;
}
// Entries a pass of the pop loop reads together (pop_batch.h).  Every fused instantiation takes it: none pays for the wider read with scratch
// memory, spilled registers or VGPRs at 2 or 3 ("Pops in batches": N = 2, 3, 4 alternated on the box; 1 is the one-entry loop)
#ifndef PT_FUSED_POP_N
#define PT_FUSED_POP_N 3
#endif
static_assert(PT_FUSED_POP_N >= 1 && PT_FUSED_POP_N <= PT_FUSED_POP_N_MAX, "pop_first_within: 1 .. 4 entries per pass");
static_assert(fused_lds_covers_leaf_read(1, 1) && fused_lds_covers_leaf_read(1, 2) && fused_lds_covers_leaf_read(21, 36) && fused_lds_covers_leaf_read(85, 85),
              "k_fused: s_shade directly behind s_tri (pair_leaf.h LOAD_D_FIRST), tables at LDS byte 0");

// PAIRS: every leaf is one triangle or one fan pair (k_extend_lds7p's trees); else leaves of up to four triangles (k_extend_lds7's)
// MODE 0: one sample group (a slot is a pixel's whole frame; radiance added in LDS); 1: several groups (every slot logs its radiance terms);
// 2: HEAD + TAIL (wavefront_types.h RenderConst::tail) -- head slots like mode 0 for samples [0, head_samples), handed out first, then one-sample tail
// slots like mode 1: what a launch of few frames ends with is short work, and only the tail's terms go through the log
// The node loop of a pass ends once fewer than B / A of the wave's tracing lanes still descend (the others hold a leaf or are done).  1080p Cornell,
// 16 / 4 frames per call, ms: 1/2 85.7 / 22.4, 2/5 85.2 / 22.2, 1/3 84.4 / 22.0, 2/7 84.3 / 22.0, 1/4 84.0 / 21.9, 1/5 84.3 / 22.0, 1/6 (rounds 4 - 5)
// 84.8 / 22.1, 1/8 85.7 / 22.4, 1/12 86.9 / 22.7, never (1/64) 96.1 / 24.9 (profiles/r05zs_node_exit.log)
// Round 6, with the loops on the wave's condition (a pass of the node loop got cheaper than a pass of the outer loop): 1/2 64.4, 2/5 63.95, 1/3 63.85, 1/4 64.1,
// 1/5 64.5, 1/8 66.0 ms per 16 frames (profiles/r06z_ab_node_exit.log): 1/3
#ifndef PT_FUSED_NODE_EXIT
#define PT_FUSED_NODE_EXIT 3
#endif
#ifndef PT_FUSED_NODE_EXIT_B
#define PT_FUSED_NODE_EXIT_B 1
#endif
// COUNT (PT_FLAG_COUNT_VISITS on the fused pipeline; never timed): every block of the loop counts its wave executions and the lanes inside them
// (FusedBlock below) -- with the blocks' instruction counts in the shipped ISA (scripts/isa_regions.py) that is where the kernel's VALU
// instructions go and which block runs at how many of its 64 lanes.  The product instantiations (COUNT = false) carry none of it.
enum FusedBlock : int {
    FB_ITER = 0,   // one pass of the outer loop (its head: the ballots that decide what runs)
    FB_SHADE,      // the shade block ran (lanes: those inside it, with a hit or asking for a slot)
    FB_HIT,        // (1) state loads of the lanes with a hit record
    FB_MISS,       // ... miss.rmiss: weight * env -- the lanes are counted; the product kernel has no code of its own for it (FB_SURFACE's runs it; NEE has)
    FB_SURFACE,    // ... closesthit.rchit: the shading record (a triangle's, or the miss record), weight * Ke (lanes: the surface hits)
    FB_ADD,        // ... color += (LDS accumulator or term log)
    FB_BOUNCE,     // ... position, tangent frame, direction, brdf * cos / pdf (raygen.rgen:77-80)
    FB_NEXT,       // ... path ended: next sample of the slot, or the slot is complete
    FB_DONE,       // ... the slot's radiance goes to memory
    FB_HANDOUT,    // (2) the wave-uniform slot hand-out ran (lanes: those asking for a slot)
    FB_DRAW,       // ... the wave drew a batch of slots (the atomic and the tile words)
    FB_TAKE,       // ... lanes that took a slot (decode slot -> frame, pixel)
    FB_CULLED,     // ... of them: the pixel cannot see the scene, the slot is finished here
    FB_PRIMARY,    // (3) camera ray of a sample (raygen.rgen:45-60)
    FB_SETUP,      // (4) state back to LDS, ray set-up for the walk
    FB_NODE,       // one BVH4 node step
    FB_POP,        // one iteration of the stack-pop loop (inside node steps and behind leaf steps)
    FB_LEAF,       // one leaf step (a triangle or a fan pair)
    FB_DIV,        // ... its divide block (a lane is inside a triangle's edges)
    FB_FINISH,     // a walk ended (cur == DONE)
    FB_TRACE,      // (no code of its own) once per pass with a walk: the lanes that trace
    FB_SPAWN,      // the steps a bounce and a camera ray share: two rand, one square root
    FB_PTARGET,    // camera ray: pixel + jitter -> target - origin, its squared length (raygen.rgen:51-56)
    FB_PDIR,       // camera ray: the normalisation's three quotients (raygen.rgen:57)
    FB_POPTOP,     // a node step whose four children all missed takes the stack's top entry, read with the node, from a register
    FB_SKIP,       // (no code of its own) lanes whose walk left out the leaf of the triangle their ray started on (self_leaf.h): once per such ray
    FB_N
};
// NEE: next-event estimation (the oracle's `nee` mode, k_shade<.., NEE>): emission at the camera ray's hit only; at every hit before the last
// one light sample (ptn::nee_sample, three random numbers before the bounce's two) whose shadow ray this lane walks next -- an any-hit walk up to
// the sample's own tmax -- then the bounce.  Per sample the adds are the depth-0 emission, the light samples hit by hit, env at the miss: the
// oracle's order.  One sample group only (MODE 0).
// LOG (pt_render_guided, fused_guided.hip): the shade block stores the first hit of every camera ray -- {best_pos, bits(best_t)}, a miss as PT_MISS --
// at gd_log_index (guided_kernel.h): k_aov_reduce's input order per frame of the launch.  No LDS, no accumulator; the instantiations with LOG =
// false carry none of it.
// RAYS (pt_radiance_device with PT_RADIANCE_FUSED, fused_rays.hip): a slot is one sample of one of the CALLER's rays, not a pixel's frame.  The
// hand-out knows no tiles -- hand-out position -> slot -> (sample, ray) by radiance_device_kernel.h's rdf_* -- and a fresh slot loads its ray and
// takes or hashes its seed where a pixel's slot builds a camera ray: weight 1, accumulator +0, depth 0, no jitter, no normalisation, no rnd, no
// leaf left out.  Such a lane goes from step (2) straight to step (4); steps (1) and (3) carry its path as they carry a camera's.  rc.spp is 1 and
// rc.n_slots the live slots (n_slots_arg: rounded up to 64); div_frames divides by the chunk's rays.  MODE 0 only; FS_PXY and FS_MB are unused.
template <int MODE, bool PAIRS, bool COUNT, bool NEE = false, bool LOG = false, bool RAYS = false>
__device__ __forceinline__ void fused_body(RenderConst rc_arg, const uint32_t *__restrict__ tiles_arg, Radiance rad_arg,
                                           const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                           const float4 *__restrict__ g_shade4, const float4 *__restrict__ g_frame4,
                                           uint32_t n_wide, uint32_t n_tris, uint32_t slot_base_arg, uint32_t n_slots_arg,
                                           uint32_t *next_slot_arg, unsigned long long *stats_arg, int refill_arg, float tmin_arg,
                                           float tmax_arg, int lds_stack, FastDiv div_frames_arg, float self_c1_arg = 0.f,
                                           const float4 *__restrict__ lights_arg = nullptr, uint32_t n_lights_arg = 0u, float light_area_arg = 0.f,
                                           uint2 *log_arg = nullptr, RdRays rays_arg = RdRays{})
{
    constexpr uint32_t LEAF_BIT = C14_LEAF, DONE = C14_DONE;
    constexpr int POP_N = PT_FUSED_POP_N;  // entries a pass of the pop loop reads together (pop_pending below)
    constexpr bool GROUPED = MODE == 1, HYB = MODE == 2;
    // SKIP: a bounce ray leaves out the leaf of the triangle it starts on when self_leaf.h's rule says that leaf cannot yield a hit: pair-leaf trees
    // (the rule is per triangle or fan pair); the NEE instantiations, whose shadow rays start on a triangle too, stay as they were
    // ... and so does the kernel of several sample groups (MODE 1), which has no register left for the code (with it: 12 B of scratch)
    constexpr bool SKIP = PAIRS && !NEE && !GROUPED;
    static_assert(ptsl::leaf_code14(0x155u, 2u) == (C14_LEAF | (1u << 11) | 0x155u) && ptsl::CODE_BITS == C14_DONE && ptsl::CODE_NONE == 0u,
                  "self_leaf.h names leaves as the staged nodes do; the root's code stands for `none`");
    static_assert(!NEE || (MODE == 0 && !COUNT), "NEE: one sample group, no instrumented twin");
    static_assert(!LOG || !COUNT, "the first-hit log: no instrumented twin");
    static_assert(!RAYS || (MODE == 0 && !COUNT && !LOG), "caller rays: one sample per slot, no instrumented twin, no first-hit log");
    static_assert(RDF_PARTS == (uint32_t)PT_FUSED_PARTS, "radiance_device_kernel.h restates the hand-out's parts");
    // (everything the persistent loop reads: a scalar register of its own -- own_sgprs)
    const RenderConst rc = ptm::own_sgprs(rc_arg);
    const Radiance rad = ptm::own_sgprs(rad_arg);
    const FastDiv div_frames = ptm::own_sgprs(div_frames_arg);
    const uint32_t *tiles = ptm::own_sgprs(static_cast<const uint32_t *>(tiles_arg));
    uint32_t *next_slot = ptm::own_sgprs(next_slot_arg);
    unsigned long long *stats = ptm::own_sgprs(stats_arg);
    const uint32_t slot_base = ptm::own_sgprs(slot_base_arg), n_slots = ptm::own_sgprs(n_slots_arg);
    const int refill = ptm::own_sgprs(refill_arg);
    const float tmin = ptm::own_sgprs(tmin_arg), tmax = ptm::own_sgprs(tmax_arg);
    const float4 *lights = nullptr;  // NEE: the emitter table (pt_scene::d_lights: 5 float4 per emitter, cdf in .w), read through the cache
    uint32_t n_lights = 0u;
    float light_area = 0.f;
    if constexpr (NEE) {
        lights = ptm::own_sgprs(lights_arg);
        n_lights = ptm::own_sgprs(n_lights_arg);
        light_area = ptm::own_sgprs(light_area_arg);
    }
    uint2 *log = nullptr;  // LOG: the first-hit log of the launch
    if constexpr (LOG) log = ptm::own_sgprs(log_arg);
    RdRays rays{};  // RAYS: the chunk's rows and seeds
    if constexpr (RAYS) rays = ptm::own_sgprs(rays_arg);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // ---- LDS: BVH4 nodes | three permuted triangle copies | shade4 | tangent frames | stack | path state (fused_lds)
    const FusedLds lds = fused_lds(n_wide, n_tris, (uint32_t)lds_stack);
    float4 *s_wide = reinterpret_cast<float4 *>(smem + lds.wide);
    float4 *s_tri = reinterpret_cast<float4 *>(smem + lds.tri);
    float4 *s_shade = reinterpret_cast<float4 *>(smem + lds.shade);
    float4 *s_frame = reinterpret_cast<float4 *>(smem + lds.frame);
    lds_u32 *my_state = (lds_u32 *)reinterpret_cast<uint32_t *>(smem + lds.state) + threadIdx.x;
    lds_stage_nodes<FTB, true>(s_wide, g_wide, n_wide);  // (child words -> 14-bit codes: extend_kernel.h COMPACT)
    lds_stage_tris<FTB, true>(s_tri, g_tri4, n_tris, s_shade, g_shade4);  // (the kz = 2 copy is also what the shade block reads)
    // (SKIP: the spare words of a frame record's second float4 hold the triangle's self-leaf rule {thr, g | code}: staged as {the launch's limit
    // max(thr, c1 * g) for dt, the code} -- self_c1_arg, ptsl::launch_c1 of the launch's tmin, is read here and nowhere in the loop)
    for (uint32_t i = threadIdx.x; i < 2 * n_tris; i += FTB) {
        float4 v = g_frame4[i];
        if (i & 1u) {
            const uint32_t gw = __float_as_uint(v.w);
            v.z = ptsl::skip_limit(v.z, gw, self_c1_arg);
            v.w = __uint_as_float(gw & ptsl::CODE_BITS);
        }
        s_frame[i] = v;
    }
    // (a miss is record n_tris of the shade table: env where a triangle's record has its Ke -- step (1) reads it through min(pos, n_tris), PT_MISS
    // being all ones.  Its other words are never used: a miss does not bounce)
    if (threadIdx.x == 0) {
        s_shade[3 * n_tris + 0] = make_float4(0.f, 0.f, 0.f, 0.f);
        s_shade[3 * n_tris + 1] = make_float4(0.f, 0.f, rc.env[0], rc.env[1]);
        s_shade[3 * n_tris + 2] = make_float4(rc.env[2], 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const float4 *wide = s_wide, *tri4 = s_tri;
    const float4 *verts = s_tri + 6 * (size_t)n_tris;

    // (the lane's stack as the address of its top entry, over a BOTTOM entry (+0 | DONE) that every pop may take: the node step's read of the top
    // entry and both pop loops need no "empty?" compare -- LaneStack, extend_kernel.h.  Each lane writes and reads its own: no barrier)
    LaneStack<FTB, POP_N - 1> stk((lds_u32 *)reinterpret_cast<uint32_t *>(smem + lds.stack) - FTB + threadIdx.x);  // (`under`: a level below the BOTTOM entry, in the path state)
    stk.arm_bottom();
    stk.park();  // (no path yet)
    const int lane = threadIdx.x & 63;

    FusedDev dev;  // (fused_dev.h: empty in the product build)
    dev.kernel_begin();
    // COUNT: {wave executions, lanes inside} of every block, kept per wave in LDS behind the product kernel's plan (no registers: the walk keeps
    // its allocation) and added by the first active lane of the moment
    // (the wave's counters are addressed where they are used, not through a pointer kept across the loop: the twin has no register to spare for it)
    auto fb_of_wave = [&]() -> lds_u32 * { return (lds_u32 *)reinterpret_cast<uint32_t *>(smem + lds.extra) + (threadIdx.x >> 6) * (2 * FB_N); };
    if constexpr (COUNT) {
        if (lane < 2 * FB_N) fb_of_wave()[lane] = 0u;
    }
#define PT_FB(B)                                                                                        \
    if constexpr (COUNT) {                                                                              \
        const unsigned long long m_fb = __ballot(1);                                                    \
        if (lane == __ffsll((long long)m_fb) - 1) { lds_u32 *s_fb = fb_of_wave(); s_fb[2 * (B)] += 1u; s_fb[2 * (B) + 1] += (uint32_t)__popcll(m_fb); } \
    }
    // (the twin's count of a block that the product kernel runs as selects inside another block's code: the lanes for which C holds.  No region of
    // its own for scripts/isa_regions.py, which reads the markers spelled PT_FB( outside of #define lines)
#define PT_FB_IF(C, B)                                                                                  \
    if constexpr (COUNT) {                                                                              \
        if (C) { PT_FB(B) }                                                                             \
    }
    // (a lane traces a ray <=> cur != DONE: the shade block sets cur = 0 with the new ray, the walk ends with cur == DONE.  No flag is kept: a
    // loop-carried bool lives in a lane mask, and every ballot of one costs a v_cndmask + v_cmp to clear its inactive lanes -- a compare does not)
    // (the lane owns a live path -- its state is in LDS; not tracing: a hit record awaits shading -- <=> its stack pointer is not parked.
    // No flag for that either: the loop's head asks for three wave masks of it per pass, and a ballot of a flag is two vector instructions, of a
    // compare one; the masks are combined as 64-bit integers on the scalar unit)
    bool out_of_slots = false;  // wave-uniform: the slot counter ran past the end
    uint32_t n_rays_wave = 0;   // wave-uniform: rays this wave started
    uint32_t n_cull_wave = 0;   // ... of them camera rays of pixels that cannot see the scene, resolved without a walk
    uint32_t w_next = 0, w_end = 0, w_base = 0;  // wave-uniform: what is left of the wave's current batch of slots, and where it began
    uint32_t w_part = blockIdx.x % (uint32_t)PT_FUSED_PARTS, w_tried = 0;  // ... the part of the slot range it draws from, parts found empty
    bool w_tails = false;       // wave-uniform, MODE 2: the head slots are all handed out, the wave draws tail slots (a second set of eight counters)
    const uint32_t n_tail_slots = HYB ? rc.lanes_active * rc.tail * rc.slots_per_lane : 0u;  // ... of this launch (n_slots: its head slots)
    // several groups: the slot range is cut into PT_FUSED_PARTS contiguous parts.  One group: part p is every PT_FUSED_PARTS-th 64-slot chunk
    // of the HAND-OUT order -- tile-major, all frames of a tile before the next tile (chunk q = tile q / frames, frame q % frames) -- so every part,
    // like the whole launch, runs from the image's centre to its border (film_work.hip numbers the tiles that way) and ENDS with border pixels of
    // all frames: slots of 32 rays where an interior one has a hundred and more.  What runs alone at the end of a launch is then short: a rank of
    // world 8 is not helped (its loss is elsewhere), 16 frames on one device are: 39.76 -> 40.8 Grays/s, two of two rounds; K = 8 +-0, K = 4 +2 %; the two-level
    // kernel loses 1 % with it and keeps the frame-major order (profiles/r04ag_ab_fused_tilemajor.log).  (Slot numbers, and with them the radiance arrays, are frame-major as before.)
    const uint32_t part_len = ((n_slots + PT_FUSED_PARTS - 1) / PT_FUSED_PARTS + 63u) & ~63u;  // (several groups)
    lds_u32 *s_wtile = (lds_u32 *)reinterpret_cast<uint32_t *>(smem + lds.wtile) + (threadIdx.x >> 6) * PT_FUSED_WTILES;
    lds_u32 *my_nee = (lds_u32 *)reinterpret_cast<uint32_t *>(smem + lds.extra) + threadIdx.x;  // (NEE)
    ptm::f3 inv{}, invf{}, on{}, of{}, orgp{};
    ptm::RayPre pre{};
    uint32_t ax = 0, ay = 0, az = 0, tri_base = 0;
    float best_t = tmax, best_V = 0.f, best_W = 0.f, best_det = 1.f;
    uint32_t best_pos = PT_MISS;
    uint32_t cur = DONE;
    // SKIP: the code of the leaf this lane's ray leaves out -- the leaf of the triangle a bounce ray starts on, where the rule allows it -- or
    // CODE_NONE (camera rays; a ray too flat for the rule).  A leaf with this code never becomes `cur`: the node step's nearest child and both pops
    // (pop_pending, the POPTOP candidate) compare with it
    // (a register of its own: riding in tri_base's spare high bits instead it cost the head + tail kernel 12 B of scratch -- DESIGN.md section 6)
    [[maybe_unused]] uint32_t self_leaf = ptsl::CODE_NONE;
    auto is_self = [&](uint32_t e) -> bool { return (e & 0x3FFFu) == self_leaf; };
    // UNDEF: values that every path writes before it reads them are declared without a fill (ptm::undef: no instruction) -- the pair-leaf kernels
    // without NEE.  The kernels of leaves of up to four and the NEE ones keep their zeros: they are short of registers where such a value has to
    // be kept (with it: 8 - 20 B more scratch in k_fused<1 | 2, false>, two to four more VGPRs in k_fused_nee)
    constexpr bool UNDEF = PAIRS && !NEE;
    auto undef_u = [] { return ptm::undef_if<UNDEF>(0u); };
    auto undef_f = [](float fill) { return ptm::undef_if<UNDEF>(fill); };

    // The stack's pop with the cull against best_t: a loop on the WAVE's condition -- the lanes that are served sit out behind one exec mask (see the
    // node loop) -- with selects inside, not branches (two more vector instructions for eight fewer scalar ones per pass).  r: PENDING for the lanes
    // that still look for an entry
    // A pass reads the top POP_N entries together (pop_batch.h: the one-entry loop's rule as a priority chain; POP_N = 1 IS that loop): it takes
    // the first of them that is within the cut, unless that one is the lane's own leaf -- then the next pass goes on below it.  One LDS round
    // trip and one turn of the loop's scalar bookkeeping for up to POP_N of the siblings that a ray pushed before a leaf step found the hit that
    // ends it: 5.80 -> 2.72 passes per 64 walked rays on the Cornell box ("Pops in batches").  At the stack's end the reads
    // below the BOTTOM entry land in the path state, which lies in front of the stack (fused_lds_covers_leaf_read); BOTTOM is within every cut
    // and comes first, so they are never taken.  A parked lane never pops.
    constexpr uint32_t PENDING = ptpb::PENDING;
    // kcut: the cut key of the moment's best_t (pop_cut or push_cut, extend_kernel.h), compared with the raw entry
    auto pop_pending = [&](uint32_t r, uint32_t kcut) -> uint32_t {
        while (__ballot(r == PENDING)) {
            if (r == PENDING) {
                PT_FB(FB_POP)
                uint32_t e[POP_N];
                stk.template peek_n<POP_N>(e);
                const ptpb::Popped p = ptpb::pop_first_within<POP_N>(e, kcut, SKIP ? self_leaf : ptpb::NO_SELF);
                if constexpr (SKIP) { PT_FB_IF(p.own, FB_SKIP) }
                if constexpr (POP_N == 1) stk.drop();
                else stk.drop_n(p.dropped);
                r = p.code;
            }
        }
        return r;
    };
    // (after a leaf step: its accept may have changed best_t, so the cut key is formed here)
    auto pop = [&]() -> uint32_t { return pop_pending(PENDING, pop_cut(best_t)); };
    // The leaf step's pop: its first pass on entries that were read WITH the leaf's vertices -- nothing is pushed during a leaf step, so they are
    // what the pop will look at, and the pass has no LDS round trip of its own.  (Not for NEE, whose accept of a shadow ray's hit clears the stack.)
    constexpr bool POP_WITH_LEAF = !NEE;
    auto pop_read = [&](const uint32_t (&e)[POP_N]) -> uint32_t {
        const uint32_t kcut = pop_cut(best_t);
        PT_FB(FB_POP)
        const ptpb::Popped p = ptpb::pop_first_within<POP_N>(e, kcut, SKIP ? self_leaf : ptpb::NO_SELF);
        if constexpr (SKIP) { PT_FB_IF(p.own, FB_SKIP) }
        if constexpr (POP_N == 1) stk.drop();
        else stk.drop_n(p.dropped);
        return pop_pending(p.code, kcut);
    };

    for (;;) {
        PT_FB(FB_ITER)
        // ---- shade block: the lanes that wait with a hit (or with nothing, while slots are left) -- once enough of them do
        const bool have = cur != DONE, path = !stk.parked();
        const unsigned long long m_have = __ballot(have), m_path = __ballot(path);
        const unsigned long long m_in_blk = ~m_have & (out_of_slots ? m_path : ~0ull);  // (waves are whole: FTB is a multiple of 64)
        const int n_work = __popcll(m_in_blk);
        if (n_work && n_work * 64 >= refill * (n_work + __popcll(m_have))) {  // (refill <= 64: a wave without a tracing lane always passes)
            // The path state of the pass: declared here, DEFINED by the step that a lane comes through -- no zero-fill for the lanes of the other steps
            // (ptm::undef: a register as it is, for no instruction).  Who writes what before which read, per lane:
            //   slot   (1) loads it (a lane with a path); (2) sets it in every branch of a lane that takes a slot.  Read by (1) itself (LOG's record,
            //          `logs` / `lslot`, rad.color / rad.nterm, the spill chain), by (2) behind its own write (finish_group / finish_plain,
            //          rad.nterm), and by (4)'s store under got_ray: a lane has got_ray only through (1) or through (2)'s in-image branch
            //   ctr    (1) loads it and rewrites it at its end; (2)'s in-image branch sets it.  Read by (3) under need_primary -- which only those two
            //          set -- and by (4)'s store
            //   pxy    (1) loads it, (2)'s in-image branch sets it; read by (3) under need_primary and by (4)'s store
            //   seed   (1) loads it; (3) sets it under need_primary BEFORE the two rnd of the spawn steps.  A bounce lane (and NEE's light sample)
            //          comes from (1).  Read by those rnd and by (4)'s store
            //   wr, wg, wb   as seed: (1) loads them, (3) sets them to 1 under need_primary; read by (1) (weight * Ke), the bounce and (4)'s store
            //   org, dir     (3) sets both for a camera ray; for a bounce it sets dir, and org (NEE: org is (1)'s, at the hit that draws the light sample
            //          or from the returning shadow ray; a shadow ray's dir is (1)'s `wi`).  Read by (4) under got_ray only
            uint32_t slot = undef_u(), ctr = undef_u(), seed = undef_u(), pxy = undef_u();
            float wr = undef_f(0.f), wg = undef_f(0.f), wb = undef_f(0.f);
            ptm::f3 org = { undef_f(0.f), undef_f(0.f), undef_f(0.f) }, dir = { undef_f(0.f), undef_f(0.f), undef_f(0.f) };
            const bool in_blk = !have && (path || !out_of_slots);
            bool got_ray = false, need_primary = false, bounce = false;
            bool freed = false;   // the lane's slot was completed in step (1): it has no path any more (what stk.parked() says, without a second compare)
            bool shadow = false;  // NEE: the lane's next ray is the shadow ray of a light sample (org, dir = the hit, wi; tmax nc.w)
            uint32_t bpos = 0u;   // NEE: the hit whose bounce step (3) draws (its position is in org)
            float4 nc{};          // NEE: the light sample's contribution | the shadow ray's tmax
            if (in_blk) { PT_FB(FB_SHADE) }
            // (1) the hit of the ray that just ended: radiance, then bounce / next sample / slot complete
            if (in_blk && path) {
                PT_FB(FB_HIT)
                slot = my_state[FS_SLOT * FTB]; ctr = my_state[FS_CTR * FTB]; seed = my_state[FS_SEED * FTB];
                wr = __uint_as_float(my_state[FS_WR * FTB]); wg = __uint_as_float(my_state[FS_WG * FTB]); wb = __uint_as_float(my_state[FS_WB * FTB]);
                if constexpr (!RAYS) pxy = my_state[FS_PXY * FTB];
                uint32_t sample = ctr & 0xFFFFu, depth = ctr >> 16;
                // raygen.rgen:76 `color += weight * emission` (adding +0 changes no bit of a non-negative accumulator, so
                // non-emitters are skipped -- as k_shade does; NaN compares false and still adds)
                float er, eg, eb;
                bool terminated, add;
                const uint32_t pos = best_pos;
                const uint32_t npos = NEE ? (uint32_t)my_nee[FS_NEE_POS * FTB] : PT_MISS;
                if constexpr (LOG) {
                    // a camera ray ended (depth 0: a NEE shadow ray returns at depth >= 1): its record, at (frame of the launch, sample, pixel of the
                    // tile list) -- the slot number decoded as the hand-out encodes it
                    if (depth == 0u) {
                        const bool tail_slot = HYB && slot >= rc.n_head;
                        const uint32_t mine = tail_slot ? slot - rc.n_head : slot - slot_base;
                        const uint32_t lane_slot = rc.div_spl.div(mine);  // = frame (one group, head slots) | frame * groups + group | frame * tail + tail j
                        const uint32_t local = mine - lane_slot * rc.slots_per_lane;
                        const uint32_t f = GROUPED ? rc.div_groups.div(lane_slot) : tail_slot ? rc.div_tail.div(lane_slot) : lane_slot;
                        ptm::st_stream<true>(log + gd_log_index(f, local, sample, rc.slots_per_lane, rc.spp), make_uint2(pos, __float_as_uint(best_t)));
                    }
                }
                if (NEE && npos != PT_MISS) {  // NEE: the shadow ray of hit npos ended -- its light sample counts if nothing was in the way; then that hit's bounce
                    er = __uint_as_float(my_nee[FS_NEE_R * FTB]); eg = __uint_as_float(my_nee[FS_NEE_G * FTB]); eb = __uint_as_float(my_nee[FS_NEE_B * FTB]);
                    add = pos == PT_MISS;
                    terminated = false;
                    bpos = npos;
                    // (the hit's position was the shadow ray's origin: the permuted copy the walk kept, put back in order -- selects, same bits)
                    org = { ptm::sel3(pre.kz, orgp.z, orgp.y, orgp.x), ptm::sel3(pre.kz, orgp.x, orgp.z, orgp.y), ptm::sel3(pre.kz, orgp.y, orgp.x, orgp.z) };
                } else if (!NEE) {
                    // miss.rmiss:10-11 / closesthit.rchit:50-65, then raygen.rgen:76: ONE sequence for both kinds of lanes.  A pass holds miss lanes and
                    // surface lanes nearly always, so a miss / surface split would run both sides and pay the masks between them; a miss reads record
                    // n_tris of the shade table (env where a triangle has its Ke: `wr * env[0]` has the same bits from LDS as from a scalar register) and
                    // ends its path by a select.  The product kernel has no miss block of its own; the twin counts the two kinds of lanes
                    if (pos != PT_MISS) { PT_FB(FB_SURFACE) }
                    PT_FB_IF(pos == PT_MISS, FB_MISS)
                    const bool miss = pos == PT_MISS;
                    const uint32_t rec = min(pos, n_tris);  // (PT_MISS is all ones)
                    const float4 s1 = s_shade[3 * rec + 1], s2 = s_shade[3 * rec + 2];
                    er = wr * s1.z; eg = wg * s1.w; eb = wb * s2.x;
                    add = miss | !(er == 0.f && eg == 0.f && eb == 0.f);  // (a miss always adds: env = 0 is a logged term too)
                    depth++;  // (a miss: its depth is set to 0 below, like that of every ended path)
                    terminated = miss | (depth >= rc.max_depth);  // raygen.rgen:62, 81-83
                } else if (pos == PT_MISS) {  // (from here: NEE) miss.rmiss:10-11 then raygen.rgen:76, 81-83
                    PT_FB(FB_MISS)
                    er = wr * rc.env[0]; eg = wg * rc.env[1]; eb = wb * rc.env[2];
                    add = true;
                    terminated = true;
                } else {
                    PT_FB(FB_SURFACE)
                    const float4 s1 = s_shade[3 * pos + 1], s2 = s_shade[3 * pos + 2];
                    er = wr * s1.z; eg = wg * s1.w; eb = wb * s2.x;
                    add = !(er == 0.f && eg == 0.f && eb == 0.f);
                    if (NEE) add = add && depth == 0u;  // (NEE: the emitters are sampled explicitly, running into one counts for camera rays only)
                    depth++;
                    terminated = depth >= rc.max_depth;  // raygen.rgen:62
                    if (NEE && !terminated) {  // (no light sample at the path's last hit: k_shade<.., NEE>)
                        // closesthit.rchit:56-57 as k_shade computes it -- the light sample's origin, then the bounce's
                        float hu, hv;
                        ptm::div2_dominant(best_V, best_W, best_det, hu, hv);
                        const float4 a = verts[3 * pos + 0], b = verts[3 * pos + 1], c = verts[3 * pos + 2];
                        const float b0 = (1.0f - hu) - hv;
                        org = { (a.x * b0 + b.x * hu) + c.x * hv, (a.y * b0 + b.y * hu) + c.y * hv, (a.z * b0 + b.z * hu) + c.z * hv };
                        bpos = pos;
                        if (n_lights) {  // three random numbers, drawn before the bounce's
                            const float4 s0 = s_shade[3 * pos + 0];
                            ptm::f3 wi;
                            shadow = ptn::nee_sample(lights, n_lights, light_area, seed, org, { s0.x, s0.y, s0.z }, s0.w, s1.x, s1.y, wr, wg, wb, wi, nc);
                            if (shadow) dir = wi;
                        }
                    }
                }
                const bool logs = GROUPED || (HYB && slot >= rc.n_head);  // (a slot whose radiance goes through the term log)
                const uint32_t lslot = HYB ? slot - rc.n_head : slot;     // ... its place in the log arrays
                const uint32_t lstride = HYB ? rc.n_tail : rc.n_slots;
                if constexpr (MODE == 0 && !NEE) {
                    // one sample group: every lane adds, without the vote.  An accumulator starts at +0 and a sum is -0 only when both terms are, so it
                    // is never -0 and `acc + (+-0)` keeps its bits: the same film as with the skip, and `add` with its three compares is dead here
                    if (add) { PT_FB(FB_ADD) }
                    my_state[FS_A * FTB] = __float_as_uint(__uint_as_float(my_state[FS_A * FTB]) + er);
                    my_state[FS_B * FTB] = __float_as_uint(__uint_as_float(my_state[FS_B * FTB]) + eg);
                    my_state[FS_C * FTB] = __float_as_uint(__uint_as_float(my_state[FS_C * FTB]) + eb);
                } else if (add) {  // (a logged term changes nterm: modes 1 and 2 keep the vote)
                    PT_FB(FB_ADD)
                    if (!logs) {
                        my_state[FS_A * FTB] = __float_as_uint(__uint_as_float(my_state[FS_A * FTB]) + er);
                        my_state[FS_B * FTB] = __float_as_uint(__uint_as_float(my_state[FS_B * FTB]) + eg);
                        my_state[FS_C * FTB] = __float_as_uint(__uint_as_float(my_state[FS_C * FTB]) + eb);
                    } else {  // the ordered term log of add_radiance (wavefront_types.h), the count kept in LDS
                        const uint32_t k = my_state[FS_A * FTB];
                        if (dbg_no_terms && k != 0xFFFFFFFFu) {}  // (fused_dev.h: false in the product build)
                        else if (k < rc.term_pcap) ptm::st_stream<true>(rad.terms + ((size_t)k * lstride + lslot), make_float4(er, eg, eb, 0.f));
                        else if (k < rc.term_cap) ptm::st_stream<true>(rad.dev->terms_over + ((size_t)lslot * (rc.term_cap - rc.term_pcap) + (k - rc.term_pcap)), make_float4(er, eg, eb, 0.f));  // (rad.dev: wavefront_types.h)
                        else {
                            const Radiance rr = *rad.dev;
                            const unsigned long long idx = atomicAdd(rr.spill_count, 1ull);
                            if (idx < rr.spill_cap) {
                                // (the slot's first pool entry ends its chain: no per-slot initialisation of the heads)
                                rr.spill[idx] = make_float4(er, eg, eb, __uint_as_float(k == rc.term_cap ? SPILL_NONE : rr.spill_head[lslot]));
                                rr.spill_head[lslot] = (uint32_t)idx;
                            } else {
                                // (not `= 1ull`: hipcc of ROCm 7.2 (AMD clang 22.0.0git), gfx950, kept that stored constant in a register pair across the whole loop, or, where
                                // it had none, in 12 B of scratch; the atomic's operand is formed here.  k_fused_inst has registers to spare and keeps the store)
                                atomicOr(rr.overflow, 1ull);
                            }
                        }
                        my_state[FS_A * FTB] = k + 1u;
                    }
                }
                if constexpr (!GROUPED && !NEE) {
                    // the path's end as selects: a pass holds ended and continuing paths nearly always.  Only a complete slot stays a branch (its
                    // store).  (Several groups keep the branch below: their `more` costs two divisions by run-time constants)
                    if (terminated) { PT_FB(FB_NEXT) }
                    bounce = !terminated;  // (the bounce itself: step (3), beside the camera rays)
                    sample += terminated ? 1u : 0u;
                    depth = terminated ? 0u : depth;
                    const bool more = RAYS ? false                                // (a caller's ray: the slot is one sample)
                                    : HYB ? (!logs && sample < rc.head_samples)  // (a tail slot is one sample)
                                          : sample < rc.spp;                      // (one group: the slot is the pixel's whole frame)
                    need_primary = terminated & more;  // the slot's next sample: raygen.rgen:45-60
                    if (terminated & !more) {  // the slot is complete
                        PT_FB(FB_DONE)
                        if (!logs) rad.color[slot] = make_float4(__uint_as_float(my_state[FS_A * FTB]), __uint_as_float(my_state[FS_B * FTB]),
                                                                   __uint_as_float(my_state[FS_C * FTB]), 0.f);
                        else if (!dbg_no_nterm) rad.nterm[lslot] = my_state[FS_A * FTB];
                        stk.park();  // (no path)
                        freed = true;
                        dev.slot_end(slot);
                    }
                } else if (!terminated) {
                    bounce = !shadow;  // (the bounce itself: step (3), beside the camera rays -- NEE: after the shadow ray, if there is one)
                    got_ray = shadow;
                } else {
                    PT_FB(FB_NEXT)
                    sample++;
                    depth = 0;
                    bool more;
                    if (RAYS) {
                        more = false;  // (a caller's ray: the slot is one sample)
                    } else if (!GROUPED) {
                        more = sample < rc.spp;  // (NEE, one group: the slot is the pixel's whole frame)
                    } else {
                        const uint32_t lane_slot = rc.div_spl.div(slot);  // = frame lane * groups + sample group (slot_pixel)
                        const uint32_t g = lane_slot - rc.div_groups.div(lane_slot) * rc.groups;
                        more = sample < min(rc.spp, (g + 1u) * rc.group_size);
                    }
                    if (more) {
                        need_primary = true;  // the slot's next sample: raygen.rgen:45-60
                    } else {  // the slot is complete
                        PT_FB(FB_DONE)
                        if (!logs) rad.color[slot] = make_float4(__uint_as_float(my_state[FS_A * FTB]), __uint_as_float(my_state[FS_B * FTB]),
                                                                   __uint_as_float(my_state[FS_C * FTB]), 0.f);
                        else if (!dbg_no_nterm) rad.nterm[lslot] = my_state[FS_A * FTB];
                        stk.park();  // (no path)
                        freed = true;
                        dev.slot_end(slot);
                    }
                }
                ctr = sample | (depth << 16);
            }
            // (2) new slots for the lanes without a path (wave-uniform part).  A wave draws PT_FUSED_BATCH consecutive slots per
            // atomic and the tile words that give them their pixels with it: the two dependent round trips to memory (~3 us) are
            // paid once per batch -- per lane and shade block, as the first version did, they were 3/4 of the kernel's time.
            const bool wants = in_blk && (!path || freed);  // (a lane in the block without a path: it asks for a slot)
            const unsigned long long m_want = __ballot(wants);
            if (m_want && !out_of_slots) {
                if (wants) { PT_FB(FB_HANDOUT) }
                if (w_next >= w_end) {
                    PT_FB(FB_DRAW)
                    // The slots are cut into PT_FUSED_PARTS contiguous parts with a counter each, 128 B apart; a wave starts on part
                    // blockIdx % 8 -- workgroups go to the eight XCDs round-robin, so the waves of one XCD share a word -- and moves
                    // on to the next part when its own is exhausted (work stealing, in ring order) until all eight are.  One word takes
                    // ~88 atomics per microsecond on this chip; shapes with many short slots (several sample groups) ask for more.
                    // One group: PT_FUSED_BATCH1 = one tile per draw (see there).  Several groups: always PT_FUSED_BATCH.
                    for (;;) {
                        // (one group: w_base / w_next / w_end count within the part)
                        const bool grp = GROUPED || (HYB && w_tails);  // (contiguous parts of the slot range, as with several groups)
                        const uint32_t ns = (HYB && w_tails) ? n_tail_slots : n_slots;
                        const uint32_t plen = HYB ? ((ns + PT_FUSED_PARTS - 1) / PT_FUSED_PARTS + 63u) & ~63u : part_len;
                        const uint32_t part_begin = grp ? w_part * plen : 0u,
                                       part_end = grp ? min(part_begin + plen, ns)
                                                      : RAYS ? rdf_part_end(ns, w_part)
                                                             : (((ns >> 6) + (uint32_t)PT_FUSED_PARTS - 1u - w_part) / (uint32_t)PT_FUSED_PARTS) << 6;
                        uint32_t rel = 0, size = 0;
                        if (lane == 0) {
                            uint32_t *cnt = next_slot + (w_part + ((HYB && w_tails) ? (uint32_t)PT_FUSED_PARTS : 0u)) * (uint32_t)PT_FUSED_PART_STRIDE;
                            size = (uint32_t)(grp ? PT_FUSED_BATCH : PT_FUSED_BATCH1);
                            rel = atomicAdd(cnt, size);
                        }
                        rel = __builtin_amdgcn_readfirstlane(rel);
                        size = __builtin_amdgcn_readfirstlane(size);
                        if (part_begin < part_end && rel < part_end - part_begin) {
                            w_base = w_next = part_begin + rel;
                            w_end = min(w_next + size, part_end);
                            break;
                        }
                        w_part = (w_part + 1u) % (uint32_t)PT_FUSED_PARTS;
                        if (++w_tried >= (uint32_t)PT_FUSED_PARTS) {
                            if (HYB && !w_tails && n_tail_slots) {  // every head slot is handed out: on to the tail slots
                                w_tails = true;
                                w_tried = 0;
                                w_part = blockIdx.x % (uint32_t)PT_FUSED_PARTS;
                                continue;
                            }
                            out_of_slots = true;
                            w_end = w_next;
                            break;
                        }
                    }
                    if (out_of_slots) dev.out_of_slots();
                    if (!RAYS && !out_of_slots && (uint32_t)lane < (w_end - w_base + 63u) / 64u) {
                        if (GROUPED || (HYB && w_tails)) {
                            const uint32_t c = slot_base + w_base + 64u * (uint32_t)lane;   // a 64-aligned chunk of slots = one 8x8 tile
                            s_wtile[lane] = tiles[(c - rc.div_spl.div(c) * rc.slots_per_lane) >> 6];
                        } else {
                            s_wtile[lane] = tiles[div_frames.div(((w_base >> 6) + (uint32_t)lane) * (uint32_t)PT_FUSED_PARTS + w_part)];
                        }
                    }
                    __builtin_amdgcn_wave_barrier();  // (a wave's LDS operations execute in order: the reads below see these words)
                }
                const uint32_t take = min((uint32_t)__popcll(m_want), w_end - w_next);
                const uint32_t rank = (uint32_t)__popcll(m_want & ((1ull << lane) - 1ull));
                uint32_t cull_n = 0u;  // samples of a slot that is finished here: its pixel cannot see the scene (RenderConst::cull)
                if (wants && rank < take) {
                    PT_FB(FB_TAKE)
                    const uint32_t mine = w_next + rank;
                    if constexpr (RAYS) {
                        // hand-out position -> slot; a slot of the launch's rounding beyond the chunk's last is nobody's.  A live one: its ray as
                        // given (rows 24 B apart, 4-byte aligned: six dword loads), its seed, then step (4)
                        slot = rdf_slot(mine, w_part);
                        if (rdf_live(slot, rc.n_slots)) {
                            uint32_t s_i, r_i;
                            rdf_sample_ray(slot, rays.m, div_frames, s_i, r_i);
                            const float *row = rays.rays6 + 6 * (size_t)r_i;
                            org = { row[0], row[1], row[2] };
                            dir = { row[3], row[4], row[5] };
                            seed = rdf_seed(rays, r_i, s_i);
                            wr = wg = wb = 1.0f;
                            ctr = 0u;  // sample 0, depth 0
                            my_state[FS_A * FTB] = 0u; my_state[FS_B * FTB] = 0u; my_state[FS_C * FTB] = 0u;  // colour = +0.0f
                            if constexpr (SKIP) self_leaf = ptsl::CODE_NONE;  // (a caller's ray may start on a triangle: tmin < t decides, as in k_extend)
                            got_ray = true;
                            dev.slot_begin();
                        }
                    } else {
                        uint32_t f, g, local;
                        if (HYB && w_tails) {  // tail slot `mine` of the launch: (frame lane, tail j, pixel); sample head_samples + j
                            const uint32_t lane_slot = rc.div_spl.div(mine);
                            f = rc.div_tail.div(lane_slot); g = lane_slot - f * rc.tail;
                            local = mine - lane_slot * rc.slots_per_lane;
                            slot = rc.n_head + mine;
                        } else if (GROUPED) {
                            slot = slot_base + mine;
                            const uint32_t lane_slot = rc.div_spl.div(slot);
                            f = rc.div_groups.div(lane_slot); g = lane_slot - f * rc.groups;
                            local = slot - lane_slot * rc.slots_per_lane;
                        } else {  // hand-out order -> slot: chunk q of the order is (tile q / frames, frame q % frames)
                            const uint32_t q = (mine >> 6) * (uint32_t)PT_FUSED_PARTS + w_part;
                            const uint32_t t = div_frames.div(q);
                            f = q - t * rc.lanes_active; g = 0u;
                            local = t * 64u + (mine & 63u);
                            slot = slot_base + f * rc.slots_per_lane + local;
                        }
                        const uint32_t tw = s_wtile[(mine - w_base) >> 6];
                        const uint32_t px = (tw & 0xFFFFu) * 8u + (local & 7u), py = (tw >> 16) * 8u + ((local >> 3) & 7u);
                        const uint32_t sample0 = (HYB && w_tails) ? rc.head_samples + g : g * rc.group_size;
                        const bool in_image = px < rc.width && py < rc.height && f < rc.lanes_active && sample0 < rc.spp;
                        if (in_image && ptc::pixel_culled(rc, px, py)) {
                            PT_FB(FB_CULLED)
                            // every sample of the slot: one camera ray, a miss, color += 1 * env -- without the walk that would find nothing (fused_cull.h)
                            if (GROUPED) cull_n = ptc::finish_group(rc, rad, slot, g);
                            else if (!(HYB && w_tails)) cull_n = ptc::finish_plain(rc, rad, slot);
                            // (head + tail: the head slot stands for ALL spp samples of such a pixel -- the same adds in the same order -- and its
                            // tail slots are nothing: k_resolve does not replay the logs of a pixel outside the rectangle)
                        } else if (in_image) {
                            pxy = px | (py << 16);
                            ctr = sample0;
                            my_state[FS_A * FTB] = 0u;  // colour.r = +0.0f | term count = 0
                            if (!GROUPED) { my_state[FS_B * FTB] = 0u; my_state[FS_C * FTB] = 0u; }
                            my_state[FS_MB * FTB] = (uint32_t)((int32_t)rc.spp * (rc.frame_base + (int32_t)f)) + 1u;
                            stk.clear_to_bottom();  // (a path)
                            need_primary = true;
                            dev.slot_begin();
                        } else if (GROUPED) {
                            rad.nterm[slot] = 0u;  // (a slot outside the image or the batch: k_resolve never reads it, kept defined anyway)
                        } else if (HYB && w_tails) {
                            rad.nterm[slot - rc.n_head] = 0u;
                        }
                    }
                }
                w_next += take;
                if (rc.cull_on) {  // (wave-uniform: the rays of the slots finished above, counted as the rays they are)
                    const uint32_t n_c = ptc::rays_finished<GROUPED>(rc, cull_n);
                    n_rays_wave += n_c;
                    n_cull_wave += n_c;
                }
            }
            // (3) the new ray: a bounce (closesthit.rchit:56-57, raygen.rgen:77-80) or the camera ray of a slot's next / first sample
            // (raygen.rgen:45-60).  Both draw two rand and take one square root -- sqrt(1 - r1^2) of the hemisphere sample, the length of the
            // camera ray's direction -- and those steps run ONCE for both kinds of lanes: the camera rays are a fifth of the rays, so a block of
            // their own ran in every shade block at ten lanes of 64 (the block table of round 6: 11 % of the kernel's instructions).  Same
            // operations on the same operands in the same order per lane: same bits.
            if (need_primary) {
                PT_FB(FB_PRIMARY)
                const uint32_t m = (ctr & 0xFFFFu) + my_state[FS_MB * FTB];  // = sample + maxSamples * frame + 1 (ptm::make_seed)
                const uint2 sd = ptm::pcg2d(make_uint2((pxy & 0xFFFFu) * m, (pxy >> 16) * m));
                seed = sd.x + sd.y;
                wr = wg = wb = 1.0f;  // raygen.rgen:59
            }
            if (bounce || need_primary) {
                PT_FB(FB_SPAWN)
                const float r1 = ptm::rnd(seed);  // bounce: cos(theta) first, azimuth second; camera ray: x jitter first, then y
                const float r2 = ptm::rnd(seed);
                // (vx, vy, vz: primary_target writes them for the camera lanes, and only those lanes' selects below take them -- a bounce lane's
                // quotient, and the guard of div3_dominant, which branches per lane, see best_V / best_W / best_det of its hit)
                float vx = undef_f(0.f), vy = undef_f(0.f), vz = undef_f(0.f), sq_arg;
                if (need_primary) {
                    PT_FB(FB_PTARGET)
                    ptm::primary_target(rc.cam, pxy & 0xFFFFu, pxy >> 16, r1, r2, vx, vy, vz);
                    sq_arg = (vx * vx + vy * vy) + vz * vz;
                } else {
                    sq_arg = 1.0f - r1 * r1;
                }
                const float sq = ptm::fsqrt(sq_arg);
                // ... and one set of quotients by a common divisor: the camera ray's direction (target - origin) / length, the bounce's barycentrics
                // (V, W) / det (closesthit.rchit:56 through the hit record's undivided numerators) -- div3_dominant serves both (the bounce's third
                // numerator is its second once more: same guard, same bits).  -1.5 %, profiles/r06w_merged_division.log
                // (The selects cost three copies: the compiler moves best_V, best_W, best_W into the operand registers for all lanes, then the camera
                // lanes overwrite them.  Camera lanes writing vx, vy straight into best_V, best_W -- their hit record is spent -- removes two of the
                // three in the listing and was 0.35 % SLOWER on the box: profiles/fused_moves_ab.json.  Left as it is.)
                float q1, q2, q3;
                [[maybe_unused]] uint32_t skip = ptsl::CODE_NONE;  // SKIP: the leaf the new ray leaves out (a camera ray starts on no triangle: none)
                ptm::div3_dominant(need_primary ? vx : best_V, need_primary ? vy : best_W, need_primary ? vz : best_W, need_primary ? sq : best_det, q1, q2, q3);
                if (need_primary) {
                    PT_FB(FB_PDIR)
                    org = { rc.cam.ox, rc.cam.oy, rc.cam.oz };
                    dir = { q1, q2, q3 };
                } else {
                    PT_FB(FB_BOUNCE)
                    const uint32_t pos = NEE ? bpos : best_pos;
                    const float4 s0 = s_shade[3 * pos + 0], s1 = s_shade[3 * pos + 1];
                    const ptm::f3 nrm = { s0.x, s0.y, s0.z };
                    const float4 f0 = s_frame[2 * pos + 0], f1 = s_frame[2 * pos + 1];
                    dir = ptm::sample_direction_frame_sq(r1, r2, sq, nrm, { f0.x, f0.y, f0.z }, { f0.w, f1.x, f1.y });
                    const float dt = (dir.x * nrm.x + dir.y * nrm.y) + dir.z * nrm.z;
                    // (the triangle's rule rides in the two spare words of its tangent-frame record: no LDS read of its own)
                    if constexpr (SKIP) skip = dt >= f1.z ? __float_as_uint(f1.w) : ptsl::CODE_NONE;  // (ptsl::skip_code with the staged limit)
                    float fr = s0.w * dt, fg = s1.x * dt, fb = s1.y * dt;
                    ptm::div3_by_pdf(fr, fg, fb);
                    wr = wr * fr; wg = wg * fg; wb = wb * fb;
                    if (!NEE) {  // (NEE: org is the hit's position already, step (1))
                        const float4 a = verts[3 * pos + 0], b = verts[3 * pos + 1], c = verts[3 * pos + 2];
                        const float hu = q1, hv = q2;
                        const float b0 = (1.0f - hu) - hv;
                        org = { (a.x * b0 + b.x * hu) + c.x * hv, (a.y * b0 + b.y * hu) + c.y * hv, (a.z * b0 + b.z * hu) + c.z * hv };
                    }
                }
                if constexpr (SKIP) self_leaf = skip;
                got_ray = true;
            }
            // (4) state back to LDS, ray set-up (the refill block of extend_body<true, false, false, true>)
            if (got_ray) {
                PT_FB(FB_SETUP)
                my_state[FS_SLOT * FTB] = slot; my_state[FS_CTR * FTB] = ctr; my_state[FS_SEED * FTB] = seed;
                my_state[FS_WR * FTB] = __float_as_uint(wr); my_state[FS_WG * FTB] = __float_as_uint(wg); my_state[FS_WB * FTB] = __float_as_uint(wb);
                if constexpr (!RAYS) my_state[FS_PXY * FTB] = pxy;
                if constexpr (NEE) {
                    my_nee[FS_NEE_POS * FTB] = shadow ? bpos : PT_MISS;
                    if (shadow) {
                        my_nee[FS_NEE_R * FTB] = __float_as_uint(nc.x); my_nee[FS_NEE_G * FTB] = __float_as_uint(nc.y); my_nee[FS_NEE_B * FTB] = __float_as_uint(nc.z);
                    }
                }
                pre = ptm::ray_setup<true>(org, dir);
                inv = { ptm::safe_inv(dir.x), ptm::safe_inv(dir.y), ptm::safe_inv(dir.z) };
                slab_setup(org, inv, invf, on, of);
                ax = inv.x < 0.f ? LDS_NEG_AXIS : 0u;
                ay = inv.y < 0.f ? LDS_NEG_AXIS : 0u;
                az = inv.z < 0.f ? LDS_NEG_AXIS : 0u;
                tri_base = (uint32_t)pre.kz * 3u * n_tris;
                orgp = { ptm::sel3(pre.kz, org.y, org.z, org.x), ptm::sel3(pre.kz, org.z, org.x, org.y), ptm::sel3(pre.kz, org.x, org.y, org.z) };
                best_t = (NEE && shadow) ? nc.w : tmax;  // (a shadow ray: its own tmax, k_extend's ray_tmax)
                // (best_V, best_W, best_det get no value of their own: the bounce of a hit -- step (3) -- and NEE's div2_dominant at a hit are their only
                // readers, both behind best_pos != PT_MISS, and the accept that sets best_pos writes all three with it -- closer_single_level's two
                // places and the loop of the leaves of up to four.  A ray that hits nothing leaves them without a value and nobody looks.  The
                // kernels without UNDEF keep the reset)
                best_V = undef_f(0.f); best_W = undef_f(0.f); best_det = undef_f(1.f);
                best_pos = PT_MISS;
                cur = 0u;
                stk.clear_to_bottom();
            }
            const uint32_t n_started = (uint32_t)__popcll(__ballot(got_ray));  // (wave-uniform control flow here: every lane keeps the same count)
            n_rays_wave += n_started;
            dev.rays_started(n_started, HYB && w_tails, lane);
        }
        // Nobody tracing, but hits pending or slots left: the shade block runs in the next pass.  The pass FALLS THROUGH the two phases (no lane
        // enters either) instead of `continue`: a second way back to the loop's head kept the hit record's old registers alive across the leaf
        // phase, and the compiler copied the five of them at every block boundary of it -- ~30 v_mov per pass (profiles/r06x_one_latch.log)
        const bool tracing = cur != DONE;
        const unsigned long long m_tracing = __ballot(tracing);
        if (m_tracing == 0ull && __ballot(!stk.parked()) == 0ull && out_of_slots) break;

        // ---- node phase (extend_body, LDS_SCENE && COMPACT): every lane descends until it holds a leaf
        const int n_have = __popcll(m_tracing);
        if (tracing) { PT_FB(FB_TRACE) }
        // The loop's condition is the WAVE's: lanes that hold a leaf sit out a pass behind one exec mask instead of leaving a divergent loop, whose
        // bookkeeping of the lanes that left cost ~15 scalar instructions per step (the scalar unit is one per CU, and this kernel kept it 70 % busy:
        // scripts/ubench/salu_rate.hip, profiles/r06z_*).  cur of a lane without a ray is DONE, which carries the leaf bit: the mask of the lanes
        // that step is one compare.  The node loop ends once fewer than PT_FUSED_NODE_EXIT_B / PT_FUSED_NODE_EXIT of the tracing lanes still descend;
        // the first step is unconditional (the vote before every step: +0.5 %; as a `for` with a first-pass flag: +4.5 %, the compiler peels it).
        {
            bool dn = cur < LEAF_BIT;  // (an inner node: the codes of leaves and DONE carry the leaf bit)
            if (__ballot(dn) != 0ull) {
                int n_cont;
                do {
                    if (dn) {
                        PT_FB(FB_NODE)
                        // (e_top, the stack's top entry read WITH the node's planes: a step whose four children all miss pushed nothing, so that entry is what
                        // its pop looks at first -- from a register instead of behind an LDS round trip: -1.8 %, profiles/r06r_speculative_pop.log.  At an
                        // empty stack the read lands on the BOTTOM entry)
                        cur = compact_node_step<FTB, false, SKIP>(wide, cur, inv, invf, on, of, ax, ay, az, tmin, best_t, stk, [&](uint32_t e_top, uint32_t kcut, [[maybe_unused]] bool skipped = false) -> uint32_t {
                            PT_FB(FB_POPTOP)
                            // (the top entry as the pop's first candidate: within the cut key -> taken -- the BOTTOM entry of an empty stack always is, and says
                            // DONE; else the loop.  SKIP: the lane's own leaf is no candidate; `skipped`: it was this step's nearest child)
                            stk.drop();
                            if constexpr (SKIP) {
                                const bool within = entry_within(e_top, kcut), self = is_self(e_top);
                                PT_FB_IF(skipped | (within & self), FB_SKIP)
                                return pop_pending((within & !self) ? (e_top & 0x3FFFu) : PENDING, kcut);
                            } else {
                                return pop_pending(entry_within(e_top, kcut) ? (e_top & 0x3FFFu) : PENDING, kcut);
                            }
                        }, is_self);
                    }
                    dn = cur < LEAF_BIT;
                    n_cont = __popcll(__ballot(dn));
                } while (n_cont * PT_FUSED_NODE_EXIT >= n_have * PT_FUSED_NODE_EXIT_B);  // (n_have >= 1 in here: no lane left ends it too)
            }
        }
        // ---- leaf phase (extend_body, PAIRS): one triangle or one fan pair per leaf
        {   // (no `if (tracing)` around it: a lane without a ray holds DONE, and one compare says "a leaf that is not DONE")
            if ((uint32_t)(cur - LEAF_BIT) < DONE - LEAF_BIT) {
                PT_FB(FB_LEAF)
                [[maybe_unused]] uint32_t e_pop[POP_N];
                if constexpr (POP_WITH_LEAF) stk.template peek_n<POP_N>(e_pop);
                // NEE: a shadow ray's range is tmin < t < its own bound, strictly -- best_t until the first hit, which ends the walk -- and tmax plays no
                // part in it (the oracle's orc_trace(..., tmin, 0.999 dist)); a path ray's ends at tmax, and a hit AT best_t goes on to the tie rule
                [[maybe_unused]] bool shadow_walk = false;
                if constexpr (NEE) shadow_walk = my_nee[FS_NEE_POS * FTB] != PT_MISS;
                if (PAIRS) {
                    const uint32_t first = cur & 0x7FFu;
                    ptl::pair_leaf_test<true, true>(tri4, (size_t)tri_base + 3 * (size_t)first, ((cur >> 11) & 3u) != 0u, first, pre, orgp, tmin, ptl::leaf_upper(NEE && shadow_walk, best_t, tmax),
                                        [&](float t, float V, float W, float det, uint32_t pos, uint32_t) {
                                            [[maybe_unused]] const bool closer =
                                                ptl::closer_single_level(tri4, tri_base, t, V, W, det, pos, best_t, best_V, best_W, best_det, best_pos);
                                            if constexpr (NEE) {  // a shadow ray: any hit below its tmax will do, nothing pending any more
                                                if (closer && my_nee[FS_NEE_POS * FTB] != PT_MISS) stk.clear_to_bottom();
                                            }
                                        },
                                        [&] { PT_FB(FB_DIV) });
                } else {
                    const uint32_t first = cur & 0x7FFu, cnt = ((cur >> 11) & 3u) + 1u;
                    for (uint32_t k = 0; k < cnt; k++) {
                        const uint32_t pos = first + k;
                        const size_t ti = (size_t)tri_base + 3 * (size_t)pos;
                        const float4 a = tri4[ti + 0], b = tri4[ti + 1], c = tri4[ti + 2];
                        float t, V, W, det;
                        if (ptm::tri_test_perm(pre, orgp, { a.x, a.y, a.z }, { b.x, b.y, b.z }, { c.x, c.y, c.z }, tmin, ptl::leaf_upper(NEE && shadow_walk, best_t, tmax), t, V, W, det, nullptr)) {
                            bool closer = t < best_t;  // closest t; equal t -> lowest gl_PrimitiveID (the first vertex of a record carries it)
                            if (!closer && t == best_t)
                                closer = best_pos == PT_MISS || __float_as_uint(a.w) < __float_as_uint(tri4[(size_t)tri_base + 3 * (size_t)best_pos].w);
                            if (closer) {
                                best_t = t; best_V = V; best_W = W; best_det = det; best_pos = pos;
                                if (NEE && my_nee[FS_NEE_POS * FTB] != PT_MISS) stk.clear_to_bottom();  // (a shadow ray: any hit will do)
                            }
                        }
                    }
                }
                if constexpr (POP_WITH_LEAF) cur = pop_read(e_pop);
                else cur = pop();
            }
            if (tracing && cur == DONE) {  // the hit (best_pos, best_V, best_W, best_det) waits in registers for the shade block
                PT_FB(FB_FINISH)
            }
        }
    }
    if (lane == 0 && n_rays_wave) atomicAdd(stats + PT_STAT_RAYS, (unsigned long long)n_rays_wave);
    if (lane == 0 && n_cull_wave) atomicAdd(stats + PT_STAT_RAYS_CULLED, (unsigned long long)n_cull_wave);  // (pt_stats.rays_culled)
    dev.kernel_end(lane, n_rays_wave, FTB);
    if constexpr (COUNT) {  // (pt_get_block_counts: stats[PT_N_STATS + 2 * block] wave executions, [+ 1] lanes inside them)
        if (lane < 2 * FB_N) atomicAdd(stats + PT_N_STATS + lane, (unsigned long long)fb_of_wave()[lane]);
    }
#undef PT_FB_IF
#undef PT_FB
}

template <int MODE, bool PAIRS>
__global__ __launch_bounds__(FTB, PT_FUSED_WAVES) void k_fused(RenderConst rc, const uint32_t *__restrict__ tiles, Radiance rad,
                                                              const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                                              const float4 *__restrict__ g_shade4, const float4 *__restrict__ g_frame4,
                                                              uint32_t n_wide, uint32_t n_tris, uint32_t slot_base, uint32_t n_slots,
                                                              uint32_t *next_slot, unsigned long long *stats, int refill, float tmin,
                                                              float tmax, int lds_stack, FastDiv div_frames, float self_c1)
{
    fused_body<MODE, PAIRS, false>(rc, tiles, rad, g_wide, g_tri4, g_shade4, g_frame4, n_wide, n_tris, slot_base, n_slots, next_slot, stats, refill, tmin,
                                   tmax, lds_stack, div_frames, self_c1);
}
// PT_FLAG_NEE: next-event estimation, one sample group; the emitter table beside the scene's (pt_scene::d_lights).  Its own LDS plan (FS_NEE_*)
// and occupancy (fused.hip); the instantiations above do not carry any of it
template <bool PAIRS>
__global__ __launch_bounds__(FTB, PT_FUSED_WAVES_NEE) void k_fused_nee(RenderConst rc, const uint32_t *__restrict__ tiles, Radiance rad,
                                                                      const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                                                      const float4 *__restrict__ g_shade4, const float4 *__restrict__ g_frame4,
                                                                      uint32_t n_wide, uint32_t n_tris, uint32_t slot_base, uint32_t n_slots,
                                                                      uint32_t *next_slot, unsigned long long *stats, int refill, float tmin,
                                                                      float tmax, int lds_stack, FastDiv div_frames,
                                                                      const float4 *__restrict__ lights, uint32_t n_lights, float light_area)
{
    fused_body<0, PAIRS, false, true>(rc, tiles, rad, g_wide, g_tri4, g_shade4, g_frame4, n_wide, n_tris, slot_base, n_slots, next_slot, stats, refill,
                                      tmin, tmax, lds_stack, div_frames, 0.f, lights, n_lights, light_area);
}
// the instrumented twin (PT_FLAG_COUNT_VISITS): the same LDS plan and block size, so a wave holds what it holds in the timed kernel; the counters
// cost registers (spills), so it is slower and never timed
template <int MODE, bool PAIRS>
__global__ __launch_bounds__(FTB, PT_FUSED_WAVES) void k_fused_count(RenderConst rc, const uint32_t *__restrict__ tiles, Radiance rad,
                                                                    const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                                                    const float4 *__restrict__ g_shade4, const float4 *__restrict__ g_frame4,
                                                                    uint32_t n_wide, uint32_t n_tris, uint32_t slot_base, uint32_t n_slots,
                                                                    uint32_t *next_slot, unsigned long long *stats, int refill, float tmin,
                                                                    float tmax, int lds_stack, FastDiv div_frames, float self_c1)
{
    fused_body<MODE, PAIRS, true>(rc, tiles, rad, g_wide, g_tri4, g_shade4, g_frame4, n_wide, n_tris, slot_base, n_slots, next_slot, stats, refill, tmin,
                                  tmax, lds_stack, div_frames, self_c1);
}
// the kernels above with the first-hit log (LOG): pt_render_guided's launches.  No instrumented twin.
template <int MODE, bool PAIRS>
__global__ __launch_bounds__(FTB, PT_FUSED_WAVES) void k_fused_log(RenderConst rc, const uint32_t *__restrict__ tiles, Radiance rad,
                                                                  const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                                                  const float4 *__restrict__ g_shade4, const float4 *__restrict__ g_frame4,
                                                                  uint32_t n_wide, uint32_t n_tris, uint32_t slot_base, uint32_t n_slots,
                                                                  uint32_t *next_slot, unsigned long long *stats, int refill, float tmin,
                                                                  float tmax, int lds_stack, FastDiv div_frames, float self_c1, uint2 *log)
{
    fused_body<MODE, PAIRS, false, false, true>(rc, tiles, rad, g_wide, g_tri4, g_shade4, g_frame4, n_wide, n_tris, slot_base, n_slots, next_slot, stats, refill,
                                                tmin, tmax, lds_stack, div_frames, self_c1, nullptr, 0u, 0.f, log);
}
template <bool PAIRS>
__global__ __launch_bounds__(FTB, PT_FUSED_WAVES_NEE) void k_fused_nee_log(RenderConst rc, const uint32_t *__restrict__ tiles, Radiance rad,
                                                                          const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                                                          const float4 *__restrict__ g_shade4, const float4 *__restrict__ g_frame4,
                                                                          uint32_t n_wide, uint32_t n_tris, uint32_t slot_base, uint32_t n_slots,
                                                                          uint32_t *next_slot, unsigned long long *stats, int refill, float tmin,
                                                                          float tmax, int lds_stack, FastDiv div_frames,
                                                                          const float4 *__restrict__ lights, uint32_t n_lights, float light_area, uint2 *log)
{
    fused_body<0, PAIRS, false, true, true>(rc, tiles, rad, g_wide, g_tri4, g_shade4, g_frame4, n_wide, n_tris, slot_base, n_slots, next_slot, stats, refill,
                                            tmin, tmax, lds_stack, div_frames, 0.f, lights, n_lights, light_area, log);
}
// the kernels of PT_RADIANCE_FUSED (RAYS): k_fused<0, PAIRS> and k_fused_nee<PAIRS> started from the caller's rays.  `tiles` is gone, `rays` is new;
// div_m divides by the chunk's rays.  Instantiated in fused_rays.hip only.
template <bool PAIRS>
__global__ __launch_bounds__(FTB, PT_FUSED_WAVES) void k_fused_rays(RenderConst rc, Radiance rad, const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                                                   const float4 *__restrict__ g_shade4, const float4 *__restrict__ g_frame4,
                                                                   uint32_t n_wide, uint32_t n_tris, uint32_t n_slots, uint32_t *next_slot,
                                                                   unsigned long long *stats, int refill, float tmin, float tmax, int lds_stack,
                                                                   FastDiv div_m, float self_c1, RdRays rays)
{
    fused_body<0, PAIRS, false, false, false, true>(rc, nullptr, rad, g_wide, g_tri4, g_shade4, g_frame4, n_wide, n_tris, 0u, n_slots, next_slot, stats, refill, tmin,
                                                    tmax, lds_stack, div_m, self_c1, nullptr, 0u, 0.f, nullptr, rays);
}
template <bool PAIRS>
__global__ __launch_bounds__(FTB, PT_FUSED_WAVES_NEE) void k_fused_nee_rays(RenderConst rc, Radiance rad, const float4 *__restrict__ g_wide,
                                                                           const float4 *__restrict__ g_tri4, const float4 *__restrict__ g_shade4,
                                                                           const float4 *__restrict__ g_frame4, uint32_t n_wide, uint32_t n_tris,
                                                                           uint32_t n_slots, uint32_t *next_slot, unsigned long long *stats, int refill,
                                                                           float tmin, float tmax, int lds_stack, FastDiv div_m,
                                                                           const float4 *__restrict__ lights, uint32_t n_lights, float light_area, RdRays rays)
{
    fused_body<0, PAIRS, false, true, false, true>(rc, nullptr, rad, g_wide, g_tri4, g_shade4, g_frame4, n_wide, n_tris, 0u, n_slots, next_slot, stats, refill, tmin,
                                                   tmax, lds_stack, div_m, 0.f, lights, n_lights, light_area, nullptr, rays);
}
