// Host driver of csrc/mt_dlog.h for tests/test_dlog_walk.py (built with
// -fsanitize=address,undefined).  Reads spans from the file named on the command line, one per
// line: "rich nw w0 w1 ...".  Each span is copied into a heap allocation of exactly nw words, so
// any load outside it is a sanitizer report, and walked twice, as the device read-out does: the
// counting sink, then -- only when the span is well formed -- the row sink.  Prints per span
// "BAD" or "OK n" followed by n rows "record seq kind position length word uid".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fluidframework_amd/csrc/mt_dlog.h"

struct Rows {
    std::vector<mt_dlog_entry> v;
    void entry(const mt_dlog_entry &e) { v.push_back(e); }
};

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int rich;
    long long nw;
    while (fscanf(f, "%d %lld", &rich, &nw) == 2) {
        int32_t *w = (int32_t *)malloc((size_t)nw * sizeof(int32_t));   // (nw == 0: no byte may be read)
        for (long long i = 0; i < nw; i++) {
            long long x;
            if (fscanf(f, "%lld", &x) != 1) return 2;
            w[i] = (int32_t)x;
        }
        mt_dlog_count c;
        if (!mt_dlog_walk(w, nw, rich != 0, c)) {
            puts("BAD");
        } else {
            Rows r;
            if (!mt_dlog_walk(w, nw, rich != 0, r) || (int64_t)r.v.size() != c.n) return 3;
            printf("OK %zu\n", r.v.size());
            for (const mt_dlog_entry &e : r.v)
                printf("%d %d %d %d %d %d %" PRIu32 "\n", e.record, e.seq, e.kind, e.position, e.length, e.word, e.uid);
        }
        free(w);
    }
    fclose(f);
    return 0;
}
