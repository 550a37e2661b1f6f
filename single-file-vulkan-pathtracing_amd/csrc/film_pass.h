// film_pass.h -- the launch shape of every per-pixel film pass (denoise.hip, reproject.hip, motion.hip, upsample.hip): a block is 64 x 4 pixels, a wave
// one row of 64, so that a wave's loads of a row are consecutive records and a row test is wave-uniform.  The constants and fp_grid compile
// for the host too (the *_kernel.h headers and the tests/*_host.cpp programs read them); fp_pixel is the device's.
// Wants declared before it: TB (pt_internal.h; tests/kernel_host.h).
#pragma once
#include <stdint.h>

constexpr int FP_BW = 64, FP_BH = TB / FP_BW;  // pixels of a block

// -> the blocks of a w x h film; *n_bx: blocks per row of blocks (what the kernels' argument structs carry)
// (a film has fewer than 2^28 pixels and sides below 2^19: far fewer than 2^31 blocks)
inline uint32_t fp_grid(uint32_t w, uint32_t h, uint32_t *n_bx)
{
    *n_bx = (w + FP_BW - 1) / FP_BW;
    return *n_bx * ((h + FP_BH - 1) / FP_BH);
}

#ifdef __HIPCC__
// The pixel of this thread.  The test against the image stays written in each kernel, `if (x >= (int)c.w || y >= (int)c.h) return;`:
// returned from here as a bool it changes the kernels' code ("Film passes").
__device__ __forceinline__ void fp_pixel(uint32_t n_bx, int &x, int &y)
{
    const uint32_t by = blockIdx.x / n_bx, bx = blockIdx.x - by * n_bx;
    x = (int)(bx * FP_BW + (threadIdx.x & (FP_BW - 1)));
    y = (int)(by * FP_BH + threadIdx.x / FP_BW);
}
#endif
