// syrk_plan_dump -- prints make_syrk_plan (csrc/gq_syrk_plan.hpp) as text for tests/test_syrk_plan_cpu.py.
//   syrk_plan_dump plan  KIND image nosplit gw ck wgs T,C,nseg ...   one launch over all the shapes, words included
//   syrk_plan_dump sweep 0    image nosplit gw ck wgs T,C,nseg ...   every shape a launch of its own (its syrk_kind), no words
// Plain host C++: g++ -std=c++17, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gq_syrk_plan.hpp"

using namespace gq;

static void dump(int kind, const SyrkShape* s, int m, const SyrkOptions& o, bool with_words) {
    const SyrkPlan p = make_syrk_plan(kind, s, m, o);
    size_t bound = 0;
    for (int k = 0; k < m; ++k) bound += syrk_workspace_bytes(s[k].T, s[k].C, o);
    printf("plan kind %d m %d total_tiles %d tl %zu per_xcd %d sp %d n_reduce %d aux_word %lld reduce_word %lld bar_word %lld "
           "ck %d nck %d img_end %zu table_off %zu partial_off %zu partial_bytes %zu grid %u block %u total %zu n_words %zu "
           "bound %zu\n",
           p.kind, p.m, p.total_tiles, p.tl, p.per_xcd, p.sp, p.n_reduce, (long long)p.aux_word, (long long)p.reduce_word,
           (long long)p.bar_word, p.ck, p.nck, p.img_end, p.table_off, p.partial_off, p.partial_bytes, p.grid, p.block, p.total,
           p.words.size(), bound);
    for (int k = 0; k < m; ++k)
        printf("problem %d T %lld C %lld syrk_kind %d Tp %lld nt %d tile_begin %d img_off %zu img_bytes %zu hs_per_seg %d "
               "seg_word %lld\n",
               k, (long long)s[k].T, (long long)s[k].C, syrk_kind(s[k].T, s[k].C, o), (long long)p.p[k].Tp, p.p[k].nt,
               p.p[k].tile_begin, p.p[k].img_off, p.p[k].img_bytes, p.p[k].hs_per_seg, (long long)p.p[k].seg_word);
    if (!with_words) return;
    printf("words");
    for (uint32_t w : p.words) printf(" %u", w);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 9 || argc - 8 > 4096) return fprintf(stderr, "usage: %s plan|sweep KIND image nosplit gw ck wgs T,C,nseg ...\n", argv[0]), 2;
    const bool sweep = !strcmp(argv[1], "sweep");
    const int kind = atoi(argv[2]), n = argc - 8;
    const SyrkOptions o{atoi(argv[3]) != 0, atoi(argv[4]) != 0, atoi(argv[5]), atoll(argv[6]), atoll(argv[7])};
    static SyrkShape s[4096];
    for (int i = 0; i < n; ++i) {
        long t, c, g;
        if (sscanf(argv[8 + i], "%ld,%ld,%ld", &t, &c, &g) != 3) return fprintf(stderr, "bad shape %s\n", argv[8 + i]), 2;
        s[i] = SyrkShape{t, c, g};
    }
    if (!sweep && n > H_MAX_GROUP) return fprintf(stderr, "at most %d problems per launch\n", H_MAX_GROUP), 2;
    if (!sweep) dump(kind, s, n, o, true);
    for (int i = 0; sweep && i < n; ++i) dump(syrk_kind(s[i].T, s[i].C, o), s + i, 1, o, false);
    return 0;
}
