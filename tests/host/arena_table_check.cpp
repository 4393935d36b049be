// Stand-alone check program of fedmlp_amd/csrc/arena_table.h's host builder (tests/test_arena_table_cpu.py compiles and runs
// it; no HIP).  Reads entry lists from stdin,
//     case NP NS n
//     kind off dense row len Ipad I Wpad W param        (n lines)
// and prints one JSON object per case and line: the refusal, or the tables arena_table_build made.
#include <cstdio>

#include "../../fedmlp_amd/csrc/arena_table.h"

int main()
{
    long long NP, NS;
    int n;
    while (scanf(" case %lld %lld %d", &NP, &NS, &n) == 3) {
        std::vector<ArenaDesc> descs;
        for (int i = 0; i < n; ++i) {
            ArenaDesc d{};
            int param;
            if (scanf("%d %lld %d %d %lld %d %d %d %d %d", &d.kind, &d.off, &d.span.dense, &d.span.row, &d.span.len, &d.Ipad, &d.I, &d.Wpad,
                      &d.W, &param) != 10)
                return 2;
            d.param = param != 0;
            descs.push_back(d);
        }
        ArenaTableHost t;
        if (const char* why = arena_table_build(descs, NP, NS, t)) {
            printf("{\"error\": \"%s\"}\n", why);
            continue;
        }
        printf("{\"error\": null, \"n_param_chunks\": %d, \"ent_of\": [", t.n_param_chunks);
        for (size_t i = 0; i < t.ent_of.size(); ++i) printf("%s%d", i ? ", " : "", t.ent_of[i]);
        printf("], \"ent\": [");
        for (size_t i = 0; i < t.ent.size(); ++i) {
            const ArenaEntry& a = t.ent[i];
            printf("%s{\"off\": %lld, \"len\": %d, \"row\": %d, \"dense\": %d, \"Ipad\": %d, \"I\": %d, \"Wpad\": %d, \"W\": %d, \"chunk0\": %d, "
                   "\"nchunks\": %d, \"all_real\": %d}",
                   i ? ", " : "", a.off, a.len, a.row, a.dense, a.Ipad, a.I, a.Wpad, a.W, a.chunk0, a.nchunks, a.all_real);
        }
        printf("], \"chunks\": [");
        for (size_t i = 0; i < t.chunks.size(); ++i)
            printf("%s[%lld, %d, %d]", i ? ", " : "", t.chunks[i].begin, t.chunks[i].len, t.chunks[i].ent);
        printf("]}\n");
    }
    return 0;
}
