// pop_batch_host.cpp -- csrc/pop_batch.h (ptpb::pop_first_within<N>: what one pass of k_fused's pop loop decides) compiled for the host and run
// over stacks read from files: what tests/test_pop_batch_cpu.py holds against the one-entry-at-a-time loop written there, plain and under the
// host's sanitizers.  The header is plain C++ and needs nothing of kernel_host.h but rd / wr.
// usage: pop_batch_host DIR  (DIR/par: n_cases depth; DIR/stack: n_cases x depth words, a case's TOP entry first; DIR/cut, DIR/self: one word per
// case.  Out, for N = 1 .. 4: DIR/o_code_N, DIR/o_pops_N (entries gone, the taken one included), DIR/o_passes_N.)
// A case is popped the way the kernel's loop does it: passes of N entries from the top until one is taken.  Every case holds a BOTTOM entry and
// at least three words below it -- what the kernel's reads under BOTTOM find in its other LDS; the test fills them with words that WOULD
// qualify -- so a pass that starts at or above BOTTOM stays inside the case, and one that starts below it is an error reported here.
#include "kernel_host.h"
#include "pop_batch.h"

template <int N>
static void run(const std::string &d, const std::vector<uint32_t> &stack, const std::vector<uint32_t> &cut, const std::vector<uint32_t> &self,
                size_t n_cases, size_t depth)
{
    std::vector<uint32_t> code(n_cases), pops(n_cases), passes(n_cases);
    for (size_t c = 0; c < n_cases; c++) {
        size_t top = 0;  // index of the top entry within the case
        uint32_t r = ptpb::PENDING, n_pass = 0;
        while (r == ptpb::PENDING) {
            if (top + N > depth) { fprintf(stderr, "case %zu: a pass of %d entries leaves the case (no BOTTOM taken)\n", c, N); exit(3); }
            uint32_t e[N];
            for (int i = 0; i < N; i++) e[i] = stack[c * depth + top + i];
            const ptpb::Popped p = ptpb::pop_first_within<N>(e, cut[c], self[c]);
            if (p.dropped < 1 || p.dropped > (uint32_t)N) { fprintf(stderr, "case %zu: dropped %u of %d\n", c, p.dropped, N); exit(3); }
            top += p.dropped;
            r = p.code;
            n_pass++;
        }
        code[c] = r; pops[c] = (uint32_t)top; passes[c] = n_pass;
    }
    const std::string s = std::to_string(N);
    wr(d + "/o_code_" + s, code); wr(d + "/o_pops_" + s, pops); wr(d + "/o_passes_" + s, passes);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: pop_batch_host DIR\n"); return 2; }
    const std::string d = argv[1];
    auto par = rd<uint32_t>(d + "/par", 2);
    const size_t n_cases = par[0], depth = par[1];
    auto stack = rd<uint32_t>(d + "/stack", n_cases * depth);
    auto cut = rd<uint32_t>(d + "/cut", n_cases), self = rd<uint32_t>(d + "/self", n_cases);
    run<1>(d, stack, cut, self, n_cases, depth);
    run<2>(d, stack, cut, self, n_cases, depth);
    run<3>(d, stack, cut, self, n_cases, depth);
    run<4>(d, stack, cut, self, n_cases, depth);
    return 0;
}
