// self_leaf.cpp -- the self-leaf rule of the fused kernel (csrc/self_leaf.h: one header for host and device) behind the host library's C-ABI,
// so that CPU tests evaluate the very functions the scene packer and the kernel use.
#include "../../include/pt_host.h"
#include "../csrc/self_leaf.h"

extern "C" {

void pth_self_leaf_rule(const float *e0, const float *e1, const float *own, const float *other, float scene_e, float *thr, uint32_t *g_bits)
{
    const ptsl::Rule r = ptsl::leaf_rule(e0, e1, own, other, scene_e);
    union { float f; uint32_t u; } v;
    v.f = r.g;
    *thr = r.thr;
    *g_bits = v.u;
}

float pth_self_leaf_c1(float tmin) { return ptsl::launch_c1(tmin); }

void pth_self_leaf_skip(const float *dt, uint32_t n, float thr, uint32_t g_word, float c1, uint32_t *code)
{
    for (uint32_t i = 0; i < n; i++) code[i] = ptsl::skip_code(dt[i], thr, g_word, c1);
}

}
