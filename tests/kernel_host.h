// kernel_host.h -- what the *_host.cpp programs put in front of a csrc/*_kernel.h header to compile a kernel's per-pixel body for the host: the
// device keywords as nothing, HIP's vector types, TB, and the IEEE operations pt_math.h's helpers are proven equal to (fdiv, div3_dominant:
// the correctly rounded quotient; fsqrt: the correctly rounded root; compile with -ffp-contract=off).  And rd / wr: an array read from / written
// to a file as a vector of exactly its size, so that an index which leaves its array is the sanitizer's to find.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <string>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct uint2 { uint32_t x, y; };
struct uchar4 { uint8_t x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
inline uchar4 make_uchar4(uint8_t a, uint8_t b, uint8_t c, uint8_t d) { return { a, b, c, d }; }
inline float4 make_float4(float a, float b, float c, float d) { return { a, b, c, d }; }
constexpr int TB = 256;
using std::min; using std::max;
namespace ptm {
struct Camera { float ox, oy, oz, tx, ty, tz, w, h, rw, rh; };
inline float fdiv(float a, float b) { return a / b; }
inline float fsqrt(float a) { return sqrtf(a); }
inline void primary_target(const Camera &cam, uint32_t px, uint32_t py, float jx, float jy, float &vx, float &vy, float &vz)
{
    const float sx = (float)px + jx, sy = (float)py + jy;
    const float qx = fdiv(sx, cam.w), qy = fdiv(sy, cam.h);
    const float dx = qx * 2.0f - 1.0f, dy = qy * 2.0f - 1.0f;
    vx = (dx + cam.tx) - cam.ox; vy = (dy + cam.ty) - cam.oy; vz = cam.tz - cam.oz;
}
inline void div3_dominant(float a1, float a2, float a3, float b, float &q1, float &q2, float &q3) { q1 = a1 / b; q2 = a2 / b; q3 = a3 / b; }
}
template <class T> std::vector<T> rd(const std::string &p, size_t n) { std::vector<T> v(n); FILE *f = fopen(p.c_str(), "rb"); if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "read %s\n", p.c_str()); exit(2); } fclose(f); return v; }
template <class T> void wr(const std::string &p, const std::vector<T> &v) { FILE *f = fopen(p.c_str(), "wb"); if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || fclose(f) != 0) { fprintf(stderr, "write %s\n", p.c_str()); exit(2); } }
