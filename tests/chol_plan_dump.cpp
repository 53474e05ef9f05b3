// chol_plan_dump -- prints make_chol_plan and make_chol_gemm_plan (csrc/gq_chol_plan.hpp) as text for
// tests/test_chol_plan_cpu.py.
//   chol_plan_dump plan p3_min b3_min planes fp32 no_pair gemm32_64_max C ...   one plan per width, words included
//   chol_plan_dump gemm planes kr lower M,N,K ...                               the stand-alone gq_chol_gemm, no words
// Plain host C++: g++ -std=c++17, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gq_chol_plan.hpp"

using namespace gq;

static long long off(size_t v) { return v == CHOL_NO_REGION ? -1 : (long long)v; }

static void dump(int64_t C, const CholOptions& o) {
    const CholPlan p = make_chol_plan(C, o);
    const CholLayout& a = p.at;
    printf("plan C %lld planes %d images %d too_many_slots %d n_steps %zu n_nodes %zu n_gemms %zu n_words %zu A %lld X %lld dead %lld "
           "zc %lld scales %lld img0 %lld img1 %lld partial %lld rmax %lld inv_scale %lld words_at %lld total %lld bound %zu\n",
           (long long)p.C, p.planes, (int)p.images, (int)p.too_many_slots, p.steps.size(), p.nodes.size(), p.gemms.size(),
           p.words.size(), off(a.A), off(a.X), off(a.dead), off(a.zc), off(a.scales), off(a.img[0]), off(a.img[1]), off(a.partial),
           off(a.rmax), off(a.inv_scale), off(a.words), off(a.total), chol_workspace_bytes(p));
    printf("steps");
    for (const CholStep& s : p.steps) printf(" %d:%d", (int)s.kind, s.at);
    printf("\n");
    for (const CholNode& n : p.nodes)
        printf("node lo %lld mid %lld hi %lld regime %d g0 %d g1 %d g2 %d\n", (long long)n.lo, (long long)n.mid, (long long)n.hi,
               (int)n.regime, n.gemm[0], n.gemm[1], n.gemm[2]);
    for (const CholGemm& g : p.gemms) {
        printf("gemm table_at %zu rlist_at %zu n_reduce %d shapes", g.table_at, g.rlist_at, g.n_reduce);
        for (const p3::GemmShape& s : g.shapes) printf(" %d,%d,%d,%d,%d", s.MT, s.NT, s.KC, s.kr, (int)s.lower);
        printf("\n");
    }
    printf("words");
    for (uint32_t w : p.words) printf(" %u", w);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc >= 9 && !strcmp(argv[1], "plan")) {
        CholOptions o{};
        o.p3_min = atoll(argv[2]);
        o.b3_min = atoll(argv[3]);
        o.planes = atoi(argv[4]);
        o.fp32 = atoi(argv[5]) != 0;
        o.no_pair = atoi(argv[6]) != 0;
        o.gemm32_64_max = atoll(argv[7]);
        for (int i = 8; i < argc; ++i) dump(atoll(argv[i]), o);
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "gemm")) {
        const int planes = atoi(argv[2]), kr = atoi(argv[3]), lower = atoi(argv[4]);
        for (int i = 5; i < argc; ++i) {
            long m, n, k;
            if (sscanf(argv[i], "%ld,%ld,%ld", &m, &n, &k) != 3) return fprintf(stderr, "bad shape %s\n", argv[i]), 2;
            const CholGemmPlan p = make_chol_gemm_plan(planes, m, n, k, kr, lower != 0);
            printf("gemm M %ld N %ld K %ld too_many_slots %d n_words %zu rlist_at %zu n_reduce %d ia %zu ib %zu partial %zu rma %zu "
                   "rmb %zu isa %zu isb %zu words_at %zu total %zu bound %zu\n",
                   m, n, k, (int)p.too_many_slots, p.words.size(), p.rlist_at, p.n_reduce, p.ia, p.ib, p.partial, p.rma, p.rmb, p.isa,
                   p.isb, p.words_at, p.total, chol_gemm_workspace_bound(m, n, k));
        }
        return 0;
    }
    return fprintf(stderr, "usage: %s plan p3_min b3_min planes fp32 no_pair gemm32_64_max C ... | gemm planes kr lower M,N,K ...\n", argv[0]), 2;
}
