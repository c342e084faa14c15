// The walk of a delta log's records (mt_get_delta_logs' rows): one function,
// instantiated by the counting pass and by the fill pass of the device read-out and, as plain
// C++, by the host test program (tests/test_dlog_walk.py).  Self-contained: no project header.
//
// A span is nw words of one document's log:
//   record  = [seq, kind, n, entry x n]
//   entry   = kind >= 0 (a delta):    [position, cachedLength]  [npd, (key, old) x max(npd, 0)]  [state]
//             kind <  0 (maintenance): [cachedLength]                                            [state]
//             (the property deltas only with kind == 2, annotate; npd < 0: undefined, no pairs)
//   state   = (rich logs only) [flags (1 marker, 2 has properties, 4 ext),
//                               marker: refType | text: (cachedLength + 1) / 2 words,
//                               np, (key, value) x max(np, 0)]
//             [ext (flags & 4): uid, position, olen, ordinal characters x max(olen, 0)]
// Every index is checked against nw before its load, and every count read from the span (n,
// npd, np, the text words, olen) against the words left before it is stepped over, in 64-bit
// arithmetic: the cursor never passes nw and never moves backwards, whatever the words hold.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MT_DLOG_HD __host__ __device__
#else
#define MT_DLOG_HD
#endif

#define MT_DLOG_NO_UID 0xFFFFFFFFu

// One delta segment as the walk sees it (mt_delta_range without its query).
struct mt_dlog_entry {
    int32_t record;     // index of the entry's record within the span (records with n == 0 count)
    int32_t seq, kind;  // the record's header
    int32_t position;   // kind >= 0: the entry's; maintenance: the ext position, else -1
    int32_t length;     // cachedLength
    int32_t word;       // the entry's first word, relative to the span
    uint32_t uid;       // the ext uid, else MT_DLOG_NO_UID
};

// Counts the entries.
struct mt_dlog_count {
    int64_t n = 0;
    MT_DLOG_HD void entry(const mt_dlog_entry &) { n++; }
};

// Calls sink.entry for every entry of w[0 .. nw) in order.  False: the span is not a whole
// number of well-formed records (the entries seen so far were still handed to the sink: a
// caller that must yield nothing for such a span counts first).
template <class Sink> MT_DLOG_HD inline bool mt_dlog_walk(const int32_t *w, int64_t nw, bool rich, Sink &sink) {
    int64_t i = 0;
    mt_dlog_entry e;
    e.record = 0;
    while (i < nw) {
        if (nw - i < 3) return false;
        e.seq = w[i];
        e.kind = w[i + 1];
        const int32_t n = w[i + 2];
        i += 3;
        if (n < 0 || n > nw - i) return false;   // (an entry is at least one word)
        for (int32_t k = 0; k < n; k++) {
            e.word = (int32_t)i;
            e.position = -1;
            e.uid = MT_DLOG_NO_UID;
            if (e.kind >= 0) {
                if (nw - i < 2) return false;
                e.position = w[i];
                e.length = w[i + 1];
                i += 2;
                if (e.kind == 2) {
                    if (nw - i < 1) return false;
                    const int32_t npd = w[i];
                    i += 1;
                    if (npd > 0) {
                        if (npd > (nw - i) / 2) return false;
                        i += 2 * (int64_t)npd;
                    }
                }
            } else {
                if (nw - i < 1) return false;
                e.length = w[i];
                i += 1;
            }
            if (rich) {
                if (nw - i < 1) return false;
                const int32_t flags = w[i];
                i += 1;
                int64_t body = 1;   // a marker's refType
                if (!(flags & 1)) {
                    if (e.length < 0) return false;
                    body = ((int64_t)e.length + 1) / 2;
                }
                if (body > nw - i) return false;
                i += body;
                if (nw - i < 1) return false;
                const int32_t np = w[i];
                i += 1;
                if (np > 0) {
                    if (np > (nw - i) / 2) return false;
                    i += 2 * (int64_t)np;
                }
                if (flags & 4) {
                    if (nw - i < 3) return false;
                    e.uid = (uint32_t)w[i];
                    if (e.kind < 0) e.position = w[i + 1];
                    const int32_t olen = w[i + 2];
                    i += 3;
                    if (olen > 0) {
                        if (olen > nw - i) return false;
                        i += olen;
                    }
                }
            }
            sink.entry(e);
        }
        e.record++;
    }
    return true;
}
