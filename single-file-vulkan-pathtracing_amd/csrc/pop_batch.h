// pop_batch.h -- the compact walk's pop over the top N entries of a lane's stack at once (k_fused's pop_pending; DESIGN.md section 6, "Pops in
// batches").
//
// The rule is the one-entry loop's: a pop takes the first entry from the top that is within the cut key (extend_kernel.h: e <= cut on the raw
// entry) and does not name the lane's own leaf (self_leaf.h; `self` = NO_SELF where the kernel has no such leaf); the entries above it are gone
// and the pointer ends one level below the taken one.
// pop_first_within<N> is one pass over N entries read together: a priority chain of selects picks the first entry WITHIN THE CUT, the top entry
// first, and drops the levels up to and including it; only that one entry is then held against `self`.  If it is the lane's own leaf, or if none
// of the N is within the cut, the pass takes nothing (PENDING) and the caller's loop goes on below what was dropped -- exactly where the
// one-entry loop would be after as many pops.  (Testing every entry against `self` inside the chain costs a mask and a compare per entry for a
// case that a ray meets at most once.)
// The BOTTOM entry (key +0 | DONE) is within every cut and is nobody's own leaf, so it is always taken where it is met; what lies below it in
// e[] -- other memory of the kernel, any words at all -- comes later in the chain and is never looked at.
//
// One header for host and device: the kernels include it through extend_kernel.h, tests/pop_batch_host.cpp compiles it alone.  Plain C++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_PB_HD __host__ __device__ __forceinline__
#else
#define PT_PB_HD inline
#endif

namespace ptpb {

constexpr uint32_t PENDING = 0xFFFFFFFFu;  // no entry taken: the lane still looks for one
constexpr uint32_t CODE_MASK = 0x3FFFu;    // an entry's 14-bit child word
constexpr uint32_t NO_SELF = 0xFFFFFFFFu;  // a `self` that no child word equals

struct Popped {
    uint32_t code;     // the taken entry's child word, or PENDING
    uint32_t dropped;  // levels the pointer goes down: up to and including the first entry within the cut, or all N
    bool own;          // that entry was within the cut and the lane's own leaf: passed over (the instrumented kernel counts it)
};

// e[0]: the top entry, e[i]: i levels below it
template <int N>
PT_PB_HD Popped pop_first_within(const uint32_t (&e)[N], uint32_t cut, uint32_t self)
{
    uint32_t raw = e[N - 1], dropped = (uint32_t)N;
    bool any = e[N - 1] <= cut;
    for (int i = N - 2; i >= 0; i--) {  // (the last select wins: the top entry's)
        const bool in = e[i] <= cut;
        raw = in ? e[i] : raw;
        dropped = in ? (uint32_t)(i + 1) : dropped;
        any |= in;
    }
    const uint32_t code = raw & CODE_MASK;
    const bool own = any & (code == self);
    return { (any & !own) ? code : PENDING, dropped, own };
}

}  // namespace ptpb
