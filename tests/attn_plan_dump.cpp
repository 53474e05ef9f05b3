// attn_plan_dump -- prints make_attn_plan (csrc/attn/gq_attn_plan.hpp) as text for tests/test_kvcache_cpu.py.
//   attn_plan_dump B Hkv cols D S ...   one line per S: S splits chunk workspace_bytes; first a line of the constants
#include <cstdio>
#include <cstdlib>

#include "attn/gq_attn_plan.hpp"

int main(int argc, char** argv) {
    using namespace gq;
    if (argc < 6) return 2;
    const int64_t B = atoll(argv[1]), Hkv = atoll(argv[2]), cols = atoll(argv[3]), D = atoll(argv[4]);
    printf("%d %d %d %d %d\n", ATTN_SUB, ATTN_TURN, ATTN_MIN_CHUNK, ATTN_MAX_SPLITS, ATTN_MAX_COLS);
    for (int i = 5; i < argc; ++i) {
        const int64_t S = atoll(argv[i]);
        const AttnPlan p = make_attn_plan(S, B, Hkv, cols);
        printf("%lld %lld %lld %zu\n", (long long)S, (long long)p.splits, (long long)p.chunk, attn_workspace_bytes(S, B, Hkv, cols, D));
    }
    return 0;
}
