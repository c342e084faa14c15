// mt_replay.hip -- HIP kernels and the C-ABI boundary (include/mt_replay.h) of the MI355X
// merge-tree replay backend.  Build: see fluidframework_amd/build.py (hipcc --offload-arch=gfx950).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mt_replay.h"
#include "mt_dlog.h"
#include "mt_kernels.h"
#include "mt_variants.h"
#ifdef MT_SINGLE_TU
#define MT_VARIANT_DEF(n, k, targs) const void *mtk_##n() { return (const void *)(k<MT_UNPAREN targs>); }
MT_VARIANTS(MT_VARIANT_DEF)
#endif

__global__ void __launch_bounds__(MT_WAVE) k_init(DevState st, const int64_t *seed_off,
                                                  const uint16_t *seed) {
    const int doc = blockIdx.x;
    if (doc >= st.n_docs) return;
    oslot_reset(st, doc);
    if (st.bslot && lane() == 0) st.bslot[doc] = -1;   // back to the main arrays
    const int64_t s0 = seed_off ? seed_off[doc] : 0, s1 = seed_off ? seed_off[doc + 1] : 0;
    const int len = (int)(s1 - s0);
    uint16_t *text = st.text + (size_t)doc * 2 * st.T;
    for (int j = lane(); j < len && j < st.T; j += MT_WAVE) text[j] = seed[s0 + j];
    if (lane() == 0) {
        init_doc_hdr(st, doc, len);
        st.retry[doc] = 0;
        // the seed segment is the root's only child: setOrdinal(child, 0) with childCount 1
        if (st.ordS) st.ordS[(size_t)doc * st.S] = 63;
        if (st.live) {   // collabWindow.localSeq 0, empty pending queue (next group id 1)
            st.live[4 * doc] = 0;
            st.live[4 * doc + 1] = 1;
            st.live[4 * doc + 2] = 0;
            st.live[4 * doc + 3] = 0;
        }
    }
}

// ---------------------------------------------------------------- summary load (config C5)
// Client.load -> SnapshotLoader.loadHeader (MT/snapshotLoader.ts:120-159): the header's
// segments become the leaves of a tree built bottom-up in blocks of MaxNodesInBlock - 1 = 7
// (reloadFromSegments MT/mergeTree.ts:1229-1284; new blocks: needsScour undefined), then
// startOrUpdateCollaboration(minSeq, seq) (MT/mergeTree.ts:1287-1304: fresh zamboni heap).
// Body segments are appended afterwards by replaying MT_F_LOAD records (mt_load_snapshots).
__global__ void __launch_bounds__(MT_WAVE) k_load_header(DevState st, const int64_t *off, const int32_t *nh,
                                                         const mt_seg_rec *segs, const uint16_t *tin,
                                                         const uint32_t *pin, const int32_t *min_seq,
                                                         const int32_t *cur_seq, LoadScratch sc, int lo) {
    // summary r of the set (off, nh, min_seq, cur_seq, sc.off index r) -> document lo + r
    const int r = blockIdx.x, doc = lo + r;
    if (doc >= st.n_docs) return;
    oslot_reset(st, doc);
    if (st.bslot && lane() == 0) st.bslot[doc] = -1;   // back to the main arrays
    const int n = nh[r];
    const mt_seg_rec *rs = segs + off[r];
    const bool big = sc.off && sc.off[2 * r] >= 0;
    uint16_t *text = st.text + (size_t)doc * 2 * st.T;
    uint32_t *props = st.props + (size_t)doc * 2 * st.P * MT_PREC;
    const int nb0 = n > 0 ? (n + MT_LOAD_FANOUT - 1) / MT_LOAD_FANOUT : 1;
    int status = !big && (n > st.S || nb0 > st.B) ? MT_DOC_CAPACITY : 0;
    const size_t B = big ? (size_t)nb0 : st.B;   // stride of a level's counts
    v4i *dA = big ? sc.A + sc.off[2 * r] : st.segA + doc * (size_t)st.S;
    u64 *dO = big ? sc.O + sc.off[2 * r] : st.segO + doc * (size_t)st.S;
    v4u *dB = big ? sc.B + sc.off[2 * r] : st.segB + doc * (size_t)st.S;
    int ttop = 0, ptop = 1;
    for (int base = 0; base < n && status == 0; base += MT_WAVE) {
        const int i = base + lane();
        const bool v = i < n;
        mt_seg_rec r;
        memset(&r, 0, sizeof(r));
        if (v) r = rs[i];
        const bool marker = (r.flags & MT_F_MARKER) != 0;
        const int tl = v && !marker ? r.len : 0;
        const int hp = v && r.props != MT_NO_PROPS ? 1 : 0;
        const int tinc = wave_scan_incl(tl), pinc = wave_scan_incl(hp);
        const int toff = ttop + tinc - tl, ph = ptop + pinc - hp;
        const int tend = ttop + bcast(tinc, MT_WAVE - 1), pend = ptop + bcast(pinc, MT_WAVE - 1);
        if (tend > st.T || pend > st.P) {
            status = MT_DOC_CAPACITY;
            break;
        }
        bool bad = false, nm = false;
        uint32_t sig = 0;   // of the stored pairs (SEGF_PSIG_MASK)
        if (hp) {   // TextSegment.make / Marker.make(props): keys with null dropped (Q5)
            const uint32_t *rec = pin + r.props;
            const uint32_t cnt = rec[0] & 0xFFFF;
            uint32_t *t = props + (size_t)ph * MT_PREC;
            uint32_t k = 0;
            for (uint32_t j = 0; j < cnt; j++) {
                if (rec[2 + 2 * j] == MT_VAL_NULL) continue;
                if (k >= MT_KMAX) {
                    bad = true;
                    break;
                }
                t[1 + 2 * k] = rec[1 + 2 * j];
                t[2 + 2 * k] = rec[2 + 2 * j];
                nm = nm || (rec[2 + 2 * j] & MT_VAL_NOMATCH_BIT) != 0;
                sig += mt_psig_mix(rec[1 + 2 * j], rec[2 + 2 * j]);
                k++;
            }
            t[0] = k;
        }
        if (ballot(bad)) {
            status = MT_DOC_CAPACITY;
            break;
        }
        // text: one wave-wide copy per segment of this chunk
        for (u64 m = ballot(tl > 0); m; m &= m - 1) {
            const int j = first_lane(m);
            const int lj = bcast(tl, j), oj = bcast(toff, j);
            const uint32_t sj = (uint32_t)bcast((int)r.payload, j);
            for (int q = lane(); q < lj; q += MT_WAVE) text[oj + q] = tin[sj + q];
        }
        if (v) {
            const bool rem = r.removed_seq != MT_RSEQ_NONE;
            uint32_t w = 0;
            if (tl > 0) w = SEGF_NL_KNOWN | (tin[r.payload + tl - 1] == '\n' ? SEGF_NL : 0u);
            if (nm) w |= SEGF_NOMATCH;
            w = psig_put(w, sig);
            dA[i] = v4i{r.len, r.seq, r.removed_seq, pack_cli(r.client, rem ? r.removed_client : 0)};
            dO[i] = 0ull;
            if (st.segP && !big) {   // no pending groups
                u64 *w = (u64 *)(st.segP + doc * (size_t)st.S + i);
                w[0] = w[1] = w[2] = w[3] = 0ull;
            }
            dB[i] = v4u{marker ? r.payload : (uint32_t)toff, hp ? (uint32_t)ph : 0u,
                        (uint32_t)(i + 1) | (marker ? MT_MARKER_BIT : 0u), w};
        }
        ttop = tend;
        ptop = pend;
    }
    // block counts, level by level (blocks of 7, the last one takes the rest)
    int nbl[MT_LV];
    int depth = 0, cnt_below = n > 0 ? n : 0, nl = nb0;
    uint8_t *cnt = big ? sc.cnt + MT_LV * sc.off[2 * r + 1] : st.cnt + (size_t)doc * MT_LV * B;
    int8_t *flg = big ? sc.flg + sc.off[2 * r + 1] : st.flg + (size_t)doc * B;
    for (int l = 0; l < MT_LV; l++) nbl[l] = 0;
    while (status == 0) {
        if (depth >= MT_LV) {
            status = MT_DOC_CAPACITY;
            break;
        }
        for (int b = lane(); b < nl; b += MT_WAVE)
            cnt[depth * B + b] = (uint8_t)min(MT_LOAD_FANOUT, cnt_below - MT_LOAD_FANOUT * b);
        nbl[depth] = nl;
        depth++;
        if (nl == 1) break;
        cnt_below = nl;
        nl = (nl + MT_LOAD_FANOUT - 1) / MT_LOAD_FANOUT;
    }
    for (int b = lane(); b < nb0 && (big || b < st.B); b += MT_WAVE) flg[b] = MT_SCOUR_UNDEF;
    if (st.ordS && !big && status == 0) {
        // reloadFromSegments ends with nodeUpdateOrdinals(root) (MT/mergeTree.ts:1273-1276):
        // child q of a block of c children gets (q + 1) * (1 << (7 - c)) - 1; children of
        // block p are [7p, 7p + c) one level down
        uint16_t *os = st.ordS + (size_t)doc * st.S;
        uint16_t *ob = st.ordB + (size_t)doc * MT_LV * st.B;
        for (int i = lane(); i < n; i += MT_WAVE) {
            const int c = cnt[i / MT_LOAD_FANOUT];
            os[i] = (uint16_t)((i % MT_LOAD_FANOUT + 1) * (1 << (7 - c)) - 1);
        }
        for (int l = 0; l + 1 < depth; l++)
            for (int b = lane(); b < nbl[l]; b += MT_WAVE) {
                const int c = cnt[(l + 1) * B + b / MT_LOAD_FANOUT];
                ob[(size_t)l * st.B + b] = (uint16_t)((b % MT_LOAD_FANOUT + 1) * (1 << (7 - c)) - 1);
            }
    }
    if (lane() == 0) {
        DocHdr h;
        memset(&h, 0, sizeof(h));
        h.n_seg = status ? 0 : n;
        h.depth = status ? 1 : depth;
        h.cur_seq = cur_seq[r];
        h.min_seq = min_seq[r];
        h.text_top = ttop;
        h.props_top = ptop;
        h.next_uid = n + 1;
        h.status = status;
        h.delta_hash = MT_FNV_OFF;
        for (int l = 0; l < MT_LV; l++) h.n_blk[l] = status ? (l == 0) : nbl[l];
        st.hdr[doc] = h;
        st.retry[doc] = 0;
    }
}

// ---------------------------------------------------------------- checksums
struct SumCtx {
    const uint32_t *props;
};
__device__ static bool same_ordered(const uint32_t *pr, uint32_t ha, uint32_t hb) {
    if (ha == 0 || hb == 0) return ha == hb;
    if (ha == hb) return true;
    const uint32_t *a = pr + (size_t)ha * MT_PREC, *b = pr + (size_t)hb * MT_PREC;
    if (a[0] != b[0]) return false;
    for (uint32_t i = 0; i < 2 * a[0]; i++)
        if (a[1 + i] != b[1 + i]) return false;
    return true;
}
__device__ static u64 fold_run(const uint32_t *pr, u64 h, uint32_t ph, int len) {
    h = fnv_u32(h, (uint32_t)len);
    h = fnv_u32(h, ph ? 1u : 0u);
    if (ph) {
        const uint32_t *p = pr + (size_t)ph * MT_PREC;
        h = fnv_u32(h, p[0]);
        for (uint32_t i = 0; i < 2 * p[0]; i++) h = fnv_u32(h, p[1 + i]);
    }
    return h;
}
// mt_checksum per document (definitions: DESIGN.md "Checksums", oracle/mt_oracle.c).
// Segment ranges of a document in document order: the flat table, or its pages.
struct SegRanges {
    const v4i *A;
    const v4u *B;
    const u64 *O;   // overlap masks (the view read-outs)
    int n;
    bool paged;
    const uint16_t *dir;
    const PageMeta *meta;
    int nr;
    __device__ int count() const { return nr; }
    __device__ void get(int r, const v4i *&a, const v4u *&b, int &cnt) const {
        if (!paged) {
            a = A;
            b = B;
            cnt = n;
            return;
        }
        const int pg = dir[r];
        a = A + (size_t)pg * MT_PG_SLOTS;
        b = B + (size_t)pg * MT_PG_SLOTS;
        cnt = meta[pg].nseg;
    }
};
__device__ static SegRanges seg_ranges(const DevState &st, int doc, const DocHdr &h) {
    SegRanges R;
    R.paged = h.pad[HDR_PAGED] != 0;
    if (R.paged) {
        const PagedBase b = doc_paged(st, doc);
        R.A = b.A;
        R.B = b.B;
        R.O = b.O;
        R.dir = b.dir;
        R.meta = b.meta;
        R.nr = h.pad[HDR_NPAGES];
        R.n = 0;
    } else {
        R.A = st.segA + doc * (size_t)st.S;
        R.B = st.segB + doc * (size_t)st.S;
        R.O = st.segO + doc * (size_t)st.S;
        R.n = h.n_seg;
        R.nr = 1;
        R.dir = nullptr;
        R.meta = nullptr;
    }
    return R;
}

// SnapshotV1.extractSync (MT/snapshotV1.ts:156-252) of a document's current state: walk the
// leaves in order; drop unacked segments and those removed at or below minSeq; coalesce runs
// of below-minSeq, unremoved segments while TextSegment.canAppend and matchProperties hold
// (MT/textSegment.ts:62-67, MT/properties.ts:61-92: the run's text is copied out once, as
// the clone + append chain builds it); everything else is emitted with its merge info.
// mode 0 counts {records, text units, props words} per document into io[3*doc]; mode 1
// writes them at the offsets io holds (the host's prefix sums).  One wave per document; the
// per-segment decisions are uniform, text copies are wave-wide.
__device__ static bool props_equal_set(const uint32_t *pr, uint32_t ha, uint32_t hb) {
    if (ha == 0 || hb == 0) return ha == hb;
    const uint32_t *a = pr + (size_t)ha * MT_PREC, *b = pr + (size_t)hb * MT_PREC;
    for (uint32_t i = 0; i < a[0]; i++)   // NaN / undefined values never match
        if (a[2 + 2 * i] & MT_VAL_NOMATCH_BIT) return false;
    for (uint32_t j = 0; j < b[0]; j++)
        if (b[2 + 2 * j] & MT_VAL_NOMATCH_BIT) return false;
    if (ha == hb) return true;
    if (a[0] != b[0]) return false;
    for (uint32_t i = 0; i < a[0]; i++) {
        bool ok = false;
        for (uint32_t j = 0; j < b[0]; j++)
            if (b[1 + 2 * j] == a[1 + 2 * i]) ok = b[2 + 2 * j] == a[2 + 2 * i];
        if (!ok) return false;
    }
    return true;
}
__global__ void __launch_bounds__(MT_WAVE) k_extract(DevState st, int mode, int64_t *io, mt_seg_rec *recs,
                                                     uint16_t *text_out, uint32_t *props_out, int32_t *win) {
    const int doc = blockIdx.x;
    if (doc >= st.n_docs) return;
    const DocHdr h = st.hdr[doc];
    const SegRanges R = seg_ranges(st, doc, h);
    const PagedBase ar = doc_paged(st, doc);   // (the arenas of the document's region)
    const uint16_t *tb = ar.text + (size_t)h.text_half * ar.T;
    const uint32_t *pr = ar.props + (size_t)h.props_half * ar.P * MT_PREC;
    const int ms = h.min_seq;
    int64_t nrec = 0, ntext = 0, nprop = 0;
    const int64_t rbase = mode ? io[3 * doc] : 0, tbase = mode ? io[3 * doc + 1] : 0, pbase = mode ? io[3 * doc + 2] : 0;
    // the coalescing candidate ("prev"): an open record
    bool open = false, p_marker = false, p_nl = false;
    int p_len = 0;
    uint32_t p_props = 0;
    int64_t p_rec = 0;
    auto emit = [&](const v4i a, const v4u b, uint32_t flags, int seq, int cli) {
        // a new record for segment (a, b); returns nothing, advances the counters
        const bool marker = (b.z & MT_MARKER_BIT) != 0;
        const int len = a.x;
        if (mode && lane() == 0) {
            mt_seg_rec r;
            memset(&r, 0, sizeof(r));
            r.len = len;
            r.seq = seq;
            r.removed_seq = a.z;
            r.client = (int16_t)cli;
            r.removed_client = a.z != MT_RSEQ_NONE ? (int16_t)seg_rcli(a) : (int16_t)0;
            r.flags = (uint8_t)(flags | (marker ? MT_F_MARKER : 0));
            r.payload = marker ? b.x : (uint32_t)(ntext);
            r.props = MT_NO_PROPS;
            if (b.y) {
                const uint32_t *src = pr + (size_t)b.y * MT_PREC;
                r.props = (uint32_t)nprop;
                uint32_t *dst = props_out + pbase + nprop;
                dst[0] = src[0];
                for (uint32_t k = 0; k < 2 * src[0]; k++) dst[1 + k] = src[1 + k];
            }
            recs[rbase + nrec] = r;
        }
        if (b.y) nprop += 1 + 2 * (int64_t)pr[(size_t)b.y * MT_PREC];
        if (!marker) {
            if (mode)
                for (int q = lane(); q < len; q += MT_WAVE) text_out[tbase + ntext + q] = tb[b.x + q];
            ntext += len;
        }
        nrec++;
    };
    for (int rr = 0; rr < R.count(); rr++) {
        const v4i *A;
        const v4u *Bv;
        int n;
        R.get(rr, A, Bv, n);
        for (int i = 0; i < n; i++) {
            const v4i a = uni4(A[i]);
            const v4u b = uni4(Bv[i]);
            const int seq = a.y, rseq = a.z;
            const bool removed = rseq != MT_RSEQ_NONE;
            // :189-191.  A live handle holds UnassignedSequenceNumber as MT_LOCAL_BASE + localSeq
            // (mt_device.h): an unacked insert and a segment whose removal is pending are elided
            // (-1 <= minSeq always holds); observer handles hold neither
            if (seq == -1 || is_local_seq(seq) || (removed && (is_local_seq(rseq) || rseq <= ms))) continue;
            const bool marker = (b.z & MT_MARKER_BIT) != 0;
            if (seq <= ms && !removed) {                                   // :196-215 coalesce
                const bool nl = !marker && a.x > 0 && tb[b.x + a.x - 1] == '\n';
                const bool can = open && !p_marker && !marker && !p_nl &&
                                 (p_len <= MT_GRAN || a.x <= MT_GRAN) && props_equal_set(pr, p_props, b.y);
                if (can) {   // prev.clone().append(segment.clone())
                    if (mode)
                        for (int q = lane(); q < a.x; q += MT_WAVE) text_out[tbase + ntext + q] = tb[b.x + q];
                    ntext += a.x;
                    p_len += a.x;
                    if (a.x > 0) p_nl = nl;   // "".endsWith("\n") leaves the run's ending
                    if (mode && lane() == 0) recs[rbase + p_rec].len = p_len;
                } else {     // pushSeg(prev); prev = segment
                    p_rec = nrec;
                    emit(a, b, 0u, 0, -2);
                    open = true;
                    p_marker = marker;
                    p_nl = nl;
                    p_len = a.x;
                    p_props = b.y;
                }
            } else {                                                        // :216-242 merge info
                open = false;
                const bool above = seq > ms;
                uint32_t f = MT_SEG_MERGE_INFO | (above ? MT_SEG_HAS_SEQ : 0u);
                emit(a, b, f, above ? seq : 0, above ? seg_cli(a) : -2);
            }
        }
    }
    if (mode == 0 && lane() == 0) {
        io[3 * doc] = nrec;
        io[3 * doc + 1] = ntext;
        io[3 * doc + 2] = nprop;
    }
    if (lane() == 0 && win) {
        win[2 * doc] = h.min_seq;
        win[2 * doc + 1] = h.cur_seq;
    }
}

// mt_checksum per document (definitions: DESIGN.md "Checksums", oracle/mt_oracle.c).
__global__ void __launch_bounds__(MT_WAVE) k_checksum(DevState st, mt_checksum *out) {
    const int doc = blockIdx.x;
    if (doc >= st.n_docs) return;
    const DocHdr h = st.hdr[doc];
    const SegRanges R = seg_ranges(st, doc, h);
    const PagedBase ar = doc_paged(st, doc);   // (the arenas of the document's region)
    const uint16_t *tb = ar.text + (size_t)h.text_half * ar.T;
    const uint32_t *pr = ar.props + (size_t)h.props_half * ar.P * MT_PREC;
    int len = 0, ntext = 0, nseg = 0;
    for (int r = 0; r < R.count(); r++) {
        const v4i *A;
        const v4u *Bv;
        int n;
        R.get(r, A, Bv, n);
        nseg += n;
        for (int base = 0; base < n; base += MT_WAVE) {
            const int i = base + lane();
            int l = 0, t = 0;
            if (i < n) {
                const v4i a = A[i];
                l = obs_len(a);
                t = (Bv[i].z & MT_MARKER_BIT) ? 0 : l;
            }
            len += wave_sum(l);
            ntext += wave_sum(t);
        }
    }
    if (lane() == 0) {
        u64 th = fnv_u32(MT_FNV_OFF, (uint32_t)ntext), hk = MT_FNV_OFF, ph = MT_FNV_OFF;
        int g = 0, run_len = 0;
        bool have = false;
        uint32_t run_p = 0;
        for (int r = 0; r < R.count(); r++) {
            const v4i *A;
            const v4u *Bv;
            int n;
            R.get(r, A, Bv, n);
            for (int i = 0; i < n; i++) {
                const v4i a = A[i];
                const v4u b = Bv[i];
                if (a.z != MT_RSEQ_NONE) continue;
                if (!(b.z & MT_MARKER_BIT)) {
                    for (int j = 0; j < a.x; j++) {
                        const uint16_t ch = tb[b.x + j];
                        hk ^= ch & 0xFF;
                        hk *= MT_FNV_PRIME;
                        hk ^= ch >> 8;
                        hk *= MT_FNV_PRIME;
                        g++;
                        if ((g & 63) == 0) {
                            th = fnv_u64(th, hk);
                            hk = MT_FNV_OFF;
                        }
                    }
                }
                if (have && same_ordered(pr, run_p, b.y)) {
                    run_len += a.x;
                } else {
                    if (have) ph = fold_run(pr, ph, run_p, run_len);
                    run_p = b.y;
                    run_len = a.x;
                    have = true;
                }
            }
        }
        if (g & 63) th = fnv_u64(th, hk);
        if (have) ph = fold_run(pr, ph, run_p, run_len);
        mt_checksum cs;
        cs.length = (uint32_t)len;
        cs.n_segments = (uint32_t)nseg;
        cs.text_hash = th;
        cs.props_hash = ph;
        cs.delta_hash = h.delta_hash;
        out[doc] = cs;
    }
}

// ---------------------------------------------------------------- bulk text read-out
// MergeTreeTextHelper.getText(currentSeq, local client, placeholder, start, end)
// (MT/textSegment.ts:154-186, gatherText :241-263) for many (doc, start, end) queries: one
// wave per query, the document's segments in chunks of 64 (one lane per segment).  A
// segment at observer position pos of visible length l gives the units [max(pos, start),
// min(pos + l, end)) -- text.substring(start - pos, end - pos) -- and a marker in the range
// gives marker_unit (nothing when 0).  end < 0: the document's length; both ends clamp.
struct TextQuery {
    int doc, s, e;
};
__device__ static TextQuery text_query(const DevState &st, int q, const uint32_t *docs, const int32_t *start,
                                       const int32_t *end) {
    TextQuery Q;
    Q.doc = docs ? (int)docs[q] : q;
    Q.s = start ? max(start[q], 0) : 0;
    const int e = end ? end[q] : -1;
    Q.e = e < 0 ? 0x7FFFFFFF : e;
    if (Q.doc < 0 || Q.doc >= st.n_docs) Q.e = 0;   // (the host refuses these)
    return Q;
}
// lane's segment i of a chunk clipped to [s, e): units it contributes, its first unit's offset
// in the arena half (-1: a marker); pos is the chunk's first position, advanced past it
__device__ __forceinline__ int text_clip(const v4i *A, const v4u *Bv, int i, int n, int s, int e, int marker_unit,
                                         int &pos, int &src) {
    int l = 0;
    uint32_t toff = 0;
    bool marker = false;
    if (i < n) {
        l = obs_len(A[i]);
        const v4u b = Bv[i];
        marker = (b.z & MT_MARKER_BIT) != 0;
        toff = b.x;
    }
    const int incl = wave_scan_incl(l);
    const int p0 = pos + incl - l;
    pos += __builtin_amdgcn_readlane(incl, 63);
    const int lo = max(p0, s), hi = min(p0 + l, e);
    int units = max(hi - lo, 0);
    if (marker) units = marker_unit ? units : 0;
    src = marker ? -1 : (int)toff + (lo - p0);
    return units;
}
__global__ void __launch_bounds__(MT_WAVE) k_text_count(DevState st, int nq, const uint32_t *docs, const int32_t *start,
                                                        const int32_t *end, int marker_unit, int64_t *len) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const TextQuery Q = text_query(st, q, docs, start, end);
    int total = 0;
    if (Q.s < Q.e) {
        const DocHdr h = st.hdr[Q.doc];
        const SegRanges R = seg_ranges(st, Q.doc, h);
        int pos = 0;
        for (int r = 0; r < R.count() && pos < Q.e; r++) {
            const v4i *A;
            const v4u *Bv;
            int n;
            R.get(r, A, Bv, n);
            for (int base = 0; base < n && pos < Q.e; base += MT_WAVE) {
                int src;
                total += text_clip(A, Bv, base + lane(), n, Q.s, Q.e, marker_unit, pos, src);
            }
        }
        total = wave_sum(total);
    }
    if (lane() == 0) len[q] = total;
}
// off[0..n]: exclusive prefix sums of len[0..n) (one block; the device variant's offsets)
__global__ void __launch_bounds__(1024) k_text_scan(const int64_t *len, int n, int64_t *off) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024;
    const int lo = min(t * per, n), hi = min(lo + per, n);
    int64_t s = 0;
    for (int i = lo; i < hi; i++) s += len[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int i = lo; i < hi; i++) {
        off[i] = run;
        run += len[i];
    }
    if (t == 1023) off[n] = part[1023];
}
// Writes query q's units at out[off[q] ..).  Per chunk the 64 clipped segments' destination
// offsets (a wave scan) and sources go to LDS and the chunk's output units are dealt across
// the lanes, which find their unit's segment by a 6-step search of the offsets: lanes follow
// output units, so short segments keep the wave busy.  In the body a lane produces the two
// units of a 4-byte-aligned destination word and stores one dword; a chunk that ends on the
// first half of a word carries that unit into the next one, so single units are stored only at
// a query's odd head and its tail.
// kPerSeg: the k_extract-style copy instead (a wave loop per segment, unit stores), kept for
// the A/B in tools/readout_probe.py.
template <bool kPerSeg>
__global__ void __launch_bounds__(MT_WAVE) k_text_gather(DevState st, int nq, const uint32_t *docs,
                                                         const int32_t *start, const int32_t *end, int marker_unit,
                                                         const int64_t *off, uint16_t *out) {
    __shared__ int s_dst[MT_WAVE], s_src[MT_WAVE];
    const int q = blockIdx.x;
    if (q >= nq) return;
    const TextQuery Q = text_query(st, q, docs, start, end);
    if (Q.s >= Q.e || off[q + 1] == off[q]) return;
    const DocHdr h = st.hdr[Q.doc];
    const SegRanges R = seg_ranges(st, Q.doc, h);
    const PagedBase ar = doc_paged(st, Q.doc);   // (the arenas of the document's region)
    const uint16_t *tb = ar.text + (size_t)h.text_half * ar.T;
    const uint32_t T = (uint32_t)ar.T;
    uint16_t *o = out + off[q];
    const int64_t room = off[q + 1] - off[q];    // never write past the query's slot
    const int odd = (int)(((uintptr_t)o >> 1) & 1);   // the slot starts on the second half of a word
    // unit u of the chunk (units of segment sg start at s_dst[sg])
    auto unit_at = [&](int u) -> uint32_t {
        int sg = 0;
#pragma unroll
        for (int step = MT_WAVE / 2; step > 0; step >>= 1)
            if (s_dst[sg + step] <= u) sg += step;
        const int sr = s_src[sg];
        if (sr < 0) return (uint32_t)marker_unit;
        const uint32_t ix = (uint32_t)sr + (uint32_t)(u - s_dst[sg]);
        return ix < T ? tb[ix] : 0u;
    };
    int pos = 0;
    int64_t done = 0;        // units of the query produced so far (the carried one included)
    bool carry = false;      // unit done - 1 is the first half of a word not yet stored
    uint32_t carry_v = 0;
    for (int r = 0; r < R.count() && pos < Q.e; r++) {
        const v4i *A;
        const v4u *Bv;
        int n;
        R.get(r, A, Bv, n);
        for (int base = 0; base < n && pos < Q.e; base += MT_WAVE) {
            int src;
            const int units = text_clip(A, Bv, base + lane(), n, Q.s, Q.e, marker_unit, pos, src);
            const int incl = wave_scan_incl(units);
            int tot = __builtin_amdgcn_readlane(incl, 63);
            if (done + tot > room) tot = (int)(room - done);   // (the state cannot change between the passes)
            if (tot <= 0) continue;
            if constexpr (kPerSeg) {
                for (int sg = 0; sg < MT_WAVE; sg++) {
                    const int un = bcast(units, sg), d0 = bcast(incl, sg) - un, sr = bcast(src, sg);
                    for (int k = lane(); k < un && d0 + k < tot; k += MT_WAVE) {
                        const uint32_t ix = (uint32_t)sr + (uint32_t)k;
                        o[done + d0 + k] = sr < 0 ? (uint16_t)marker_unit : (ix < T ? tb[ix] : (uint16_t)0);
                    }
                }
                done += tot;
                continue;
            }
            __syncthreads();   // the previous chunk's readers are done with the LDS arrays
            s_dst[lane()] = incl - units;
            s_src[lane()] = src;
            __syncthreads();
            // chunk-local unit u lies at o[done + u]; u = -1 is the carried unit
            int u0 = carry ? -1 : 0;
            if (!carry && ((done + odd) & 1)) {   // the query's odd head (done == 0 here)
                if (lane() == 0) o[done] = (uint16_t)unit_at(0);
                u0 = 1;
            }
            const int npair = (tot - u0) >> 1;
            for (int k = lane(); k < npair; k += MT_WAVE) {
                const int u = u0 + 2 * k;
                const uint32_t a = u < 0 ? carry_v : unit_at(u), b = unit_at(u + 1);
                *(uint32_t *)(o + done + u) = a | (b << 16);
            }
            carry = ((tot - u0) & 1) != 0;
            if (carry) carry_v = unit_at(tot - 1);
            done += tot;
        }
    }
    if (!kPerSeg && carry && lane() == 0) o[done - 1] = (uint16_t)carry_v;   // the tail
}

// ---------------------------------------------------------------- bulk property-run read-out
// mt_get_prop_runs clipped to [start, end) for many (doc, start, end) queries: the walk of
// k_text_count (markers count one position).  A lane whose segment has a position inside the
// range contributes; it heads a run when the nearest contributing segment before it -- a lower
// lane of the chunk, else the wave-uniform carry across chunks and pages -- does not hold the
// same property set (mt_get_prop_runs' `same`: equal handles, or two records equal word for
// word).  Removed and clipped-away segments contribute nothing, so they neither break a run
// nor start one.
#define MT_PROPS_NONE 0xFFFFFFFFu   // carry: no contributing segment yet; row: no properties
struct PropsLane {
    int units;       // positions of the lane's segment inside the range
    uint32_t eh;     // its record handle (0: none; a handle >= P or a count > MT_KMAX reads as 0)
    int cnt;         // keys of that record
    bool head;       // the segment starts a run
};
__device__ __forceinline__ PropsLane props_chunk(const v4i *A, const v4u *Bv, int i, int n, const TextQuery &Q,
                                                 const uint32_t *pr, uint32_t P, int &pos, uint32_t &carry) {
    PropsLane L;
    int src;
    L.units = text_clip(A, Bv, i, n, Q.s, Q.e, 1, pos, src);
    const uint32_t ph = i < n ? Bv[i].y : 0u;
    const uint32_t hi = ph < P ? ph : 0u;
    const uint32_t c = pr[(size_t)hi * MT_PREC];
    const bool ok = (hi != 0u) & (c <= (uint32_t)MT_KMAX);
    L.eh = ok ? hi : 0u;
    L.cnt = ok ? (int)c : 0;
    const bool con = L.units > 0;
    const u64 contrib = ballot(con);
    const u64 below = contrib & ((1ull << lane()) - 1ull);
    const int pl = below ? 63 - __clzll((long long)below) : lane();
    const uint32_t got = (uint32_t)__shfl((int)L.eh, pl, MT_WAVE);
    const uint32_t prev = below ? got : carry;
    // both handles are validated ones (or the carry's "none"), so every record read is in bounds;
    // the words are loaded unconditionally and masked (no short-circuit)
    const bool cmp = con & (prev != MT_PROPS_NONE) & (prev != L.eh) & (prev != 0u) & (L.eh != 0u);
    bool eq = prev == L.eh;
    if (ballot(cmp)) {
        const uint32_t *x = pr + (size_t)(cmp ? prev : 0u) * MT_PREC, *y = pr + (size_t)(cmp ? L.eh : 0u) * MT_PREC;
        const uint32_t cx = x[0];
        uint32_t diff = cx ^ y[0];
#pragma unroll
        for (uint32_t k = 0; k < 2 * MT_KMAX; k++) {
            const uint32_t xv = x[1 + k], yv = y[1 + k];
            diff |= (k < 2u * cx ? 0xFFFFFFFFu : 0u) & (xv ^ yv);
        }
        eq = eq | (cmp & (diff == 0u));
    }
    L.head = con & !eq;
    if (contrib) carry = (uint32_t)bcast((int)L.eh, 63 - __clzll((long long)contrib));
    return L;
}
__global__ void __launch_bounds__(MT_WAVE) k_props_count(DevState st, int nq, const uint32_t *docs, const int32_t *start,
                                                         const int32_t *end, int64_t *n_runs, int64_t *n_words) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const TextQuery Q = text_query(st, q, docs, start, end);
    int runs = 0, words = 0;
    if (Q.s < Q.e) {
        const DocHdr h = st.hdr[Q.doc];
        const SegRanges R = seg_ranges(st, Q.doc, h);
        const PagedBase ar = doc_paged(st, Q.doc);   // (the arenas of the document's region)
        const uint32_t P = (uint32_t)ar.P;
        const uint32_t *pr = ar.props + (size_t)h.props_half * P * MT_PREC;
        int pos = 0;
        uint32_t carry = MT_PROPS_NONE;
        for (int r = 0; r < R.count() && pos < Q.e; r++) {
            const v4i *A;
            const v4u *Bv;
            int n;
            R.get(r, A, Bv, n);
            for (int base = 0; base < n && pos < Q.e; base += MT_WAVE) {
                const PropsLane L = props_chunk(A, Bv, base + lane(), n, Q, pr, P, pos, carry);
                runs += __popcll(ballot(L.head));
                words += (L.head & (L.eh != 0u)) ? 1 + 2 * L.cnt : 0;
            }
        }
        words = wave_sum(words);
    }
    if (lane() == 0) {
        n_runs[q] = runs;
        n_words[q] = words;
    }
}
// Writes query q's rows at runs[3 * run_off[q] ..) and its records at records[word_off[q] ..).
// A head lane writes its row's position and record offset at its rank (heads before it in the
// chunk plus the runs done) and copies its record's words (<= 17, a per-lane loop) to the
// words done plus an exclusive scan of the chunk's word counts.  Visible positions tile the
// range, so a run's length is the next head's position minus its own: inside a chunk from that
// head's lane; the chunk's last run stays open in wave-uniform state {row, position} until the
// next head, or the end of the walk, closes it.  Rows and words are checked against the
// query's slots, so a failed document's inconsistent rows cannot write outside the result.
__global__ void __launch_bounds__(MT_WAVE) k_props_gather(DevState st, int nq, const uint32_t *docs,
                                                          const int32_t *start, const int32_t *end,
                                                          const int64_t *run_off, const int64_t *word_off,
                                                          uint32_t *runs, uint32_t *records) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const TextQuery Q = text_query(st, q, docs, start, end);
    const int64_t room_r = run_off[q + 1] - run_off[q], room_w = word_off[q + 1] - word_off[q];
    if (Q.s >= Q.e || room_r <= 0) return;
    const DocHdr h = st.hdr[Q.doc];
    const SegRanges R = seg_ranges(st, Q.doc, h);
    const PagedBase ar = doc_paged(st, Q.doc);
    const uint32_t P = (uint32_t)ar.P;
    const uint32_t *pr = ar.props + (size_t)h.props_half * P * MT_PREC;
    uint32_t *rows = runs + 3 * run_off[q];
    uint32_t *rec = records + word_off[q];
    int pos = 0;
    uint32_t carry = MT_PROPS_NONE;
    int done = 0;             // positions of the range covered so far
    int64_t runs_done = 0, words_done = 0;
    int64_t open_row = -1;    // the run not yet closed, and its position
    int open_pos = 0;
    for (int r = 0; r < R.count() && pos < Q.e; r++) {
        const v4i *A;
        const v4u *Bv;
        int n;
        R.get(r, A, Bv, n);
        for (int base = 0; base < n && pos < Q.e; base += MT_WAVE) {
            const PropsLane L = props_chunk(A, Bv, base + lane(), n, Q, pr, P, pos, carry);
            const u64 hm = ballot(L.head);
            const int incl = wave_scan_incl(L.units);
            const int wc = (L.head & (L.eh != 0u)) ? 1 + 2 * L.cnt : 0;
            const int winc = wave_scan_incl(wc);
            if (hm) {
                const int p = Q.s + done + incl - L.units;   // the segment's first position inside the range
                const int64_t rank = runs_done + __popcll(hm & ((1ull << lane()) - 1ull));
                const u64 above = hm & ~((2ull << lane()) - 1ull);
                const int np = __shfl(p, above ? first_lane(above) : lane(), MT_WAVE);
                const int64_t w0 = words_done + winc - wc;
                const bool fits = (wc > 0) & (w0 + wc <= room_w);
                if (L.head && rank < room_r) {
                    uint32_t *row = rows + 3 * rank;
                    row[0] = (uint32_t)p;
                    if (above) row[1] = (uint32_t)(np - p);
                    row[2] = fits ? (uint32_t)w0 : MT_PROPS_NONE;
                }
                if (L.head && fits) {
                    const uint32_t *x = pr + (size_t)L.eh * MT_PREC;
                    rec[w0] = (uint32_t)L.cnt;
                    for (int k = 1; k < wc; k++) rec[w0 + k] = x[k];
                }
                const int fp = bcast(p, first_lane(hm)), lp = bcast(p, 63 - __clzll((long long)hm));
                if (open_row >= 0 && open_row < room_r && lane() == 0) rows[3 * open_row + 1] = (uint32_t)(fp - open_pos);
                runs_done += __popcll(hm);
                open_row = runs_done - 1;
                open_pos = lp;
            }
            done += bcast(incl, 63);
            words_done += bcast(winc, 63);
        }
    }
    if (open_row >= 0 && open_row < room_r && lane() == 0) rows[3 * open_row + 1] = (uint32_t)(Q.s + done - open_pos);
}

// ---------------------------------------------------------------- bulk ranged segment walk
// Client.walkSegments(handler, start, end) (MT/client.ts:276-285 -> MergeTree.mapRange / nodeMap,
// MT/mergeTree.ts:2830-2840, :2936-2998) for many (doc, start, end) queries in the replica's own
// view: one wave per query, the rows in chunks of 64 as k_text_count walks them.  nodeMap enters
// a child -- a block or a leaf -- when (end > 0) && (len > 0) && (start < len) holds on the start
// and end shifted by the lengths before it, so a row at observer position pos of observer length
// len is visited iff len > 0, pos < end and pos + len > start; nothing is clamped, start == end
// inside a row visits it and start > end visits the row that spans both.
// The count pass gives per query the visited rows, the units of the visited text rows (whole
// texts, not the clipped part: the handler gets the segment) and the words of their property
// records, and the query's end as the leaf action sees it (an undefined end is the document's
// length, which the walk to the document's end has summed); the gather repeats the walk.
static_assert(sizeof(mt_walk_row) == 48, "mt_walk_row size");
struct WalkQuery {         // wave-uniform
    int doc, s, e;         // e: 0x7FFFFFFF while an undefined end is not yet resolved
    bool open;             // the end is undefined (NULL or < 0)
};
__device__ static WalkQuery walk_query(const DevState &st, int q, const uint32_t *docs, const int32_t *start,
                                       const int32_t *end) {
    WalkQuery Q;
    Q.doc = docs ? (int)docs[q] : q;
    Q.s = start ? max(start[q], 0) : 0;   // (the host refuses a negative start)
    const int e = end ? end[q] : -1;
    Q.open = e < 0;
    Q.e = Q.open ? 0x7FFFFFFF : e;
    if (Q.doc < 0 || Q.doc >= st.n_docs) {   // (the host refuses these)
        Q.doc = 0;
        Q.e = 0;
        Q.open = false;
    }
    return Q;
}
// Where the walk starts: row 0, or on a paged document the first page whose inclusive
// PageMeta.obs prefix exceeds start (k_locate's directory scan, 64 positions at a time) -- every
// row before that page ends at or before start.  r0: the range (page) index, pos / rows: the
// observer length and the rows before it; no such page: r0 = the range count (nothing to visit,
// pos is the document's length).
__device__ __forceinline__ void walk_seek(const SegRanges &R, int s, int skip, int &r0, int &pos, int &rows) {
    r0 = pos = rows = 0;
    if (!R.paged || !skip) return;
    bool at = false;
    for (int base = 0; !at && base < R.nr; base += MT_WAVE) {
        const int j = base + lane();
        const bool v = j < R.nr;
        const int pg = R.dir[v ? j : 0];
        const PageMeta pm = R.meta[pg];
        const int ob = v ? pm.obs : 0, ns = v ? (int)pm.nseg : 0;
        const int oin = wave_scan_incl(ob), nin = wave_scan_incl(ns);
        const u64 m = ballot(v & (pos + oin > s));
        if (m) {
            const int l = first_lane(m);
            r0 = base + l;
            pos += bcast(oin - ob, l);
            rows += bcast(nin - ns, l);
            at = true;
        } else {
            pos += bcast(oin, 63);
            rows += bcast(nin, 63);
        }
    }
    if (!at) r0 = R.nr;
}
struct WalkLane {
    bool vis;        // the lane's row is visited
    int p0;          // its position in the view (the observer position in the replica's own)
    int units;       // text units it contributes (its whole text; 0: a marker, or text not asked for)
    int wc;          // words of its property record (0: none, or not asked for)
    v4i a;
    v4u b;
};
// The (refSeq, client) view of a query (k_walk_count<true> / k_walk_gather<true>, DESIGN section
// 26): a row's length is vl = (ins & !gone) ? len : 0 with ins / gone as loc_chunk has them, its
// partial term pl = len * (ins - gone); N = sum pl, L = sum vl.  N == L: every interior length is
// the non-negative sum of its leaves' vl and nodeMap's test on the shifted start / end is the
// flat one on the vl prefix; else the query is marked for the host (host_map).  local: the
// replica's own view (client 0), which walks as k_walk_count<false> does.
#define MT_WALKQ_HOST 1      // mark: a view with N != L, answered on the host
#define MT_WALKQ_INVALID 2   // mark: a remote refSeq outside [minSeq, currentSeq]
#define MT_WALKQ_SKIP 4      // mark: a remote walk that starts at the page the table-based seek found
struct WalkView {          // wave-uniform
    bool local;
    int r, c, cs;          // refSeq, short client, the client's overlap slot (0: none)
    const uint16_t *ovf;   // the document's overflow sets (paged documents)
    int OA;
};
template <bool kView> struct WalkViewArgs {};
template <> struct WalkViewArgs<true> {
    const int32_t *ref_seq, *client;   // [nq]
    int32_t *mark;                     // [nq]: written by the count pass, read by the gather
    int32_t *seek;                     // [nq][3]: a page-skip start {range, position, rows} (mark MT_WALKQ_SKIP)
    int lds_pages;                     // page ids the count pass's dynamic LDS array holds
};
__device__ static bool loc_ovf_member(const uint16_t *ovf, int OA, u64 o, int c);
// lane's row i of a range of n rows; pos is the chunk's first position, advanced past it.  A row
// past the count is loaded from index 0 and masked; the record's count word is loaded
// unconditionally (record 0 for a handle outside the arena) and masked, and
// so is, in a view, the row's overlap mask.  nacc: (per lane) its rows' terms of N.
template <bool kView>
__device__ __forceinline__ WalkLane walk_chunk(const v4i *A, const u64 *O, const v4u *Bv, int i, int n,
                                               const WalkQuery &Q, const WalkView &V, uint32_t what,
                                               const uint32_t *pr, uint32_t P, int &pos, int &nacc) {
    WalkLane L;
    const bool v = i < n;
    const int ic = v ? i : 0;
    L.a = A[ic];
    L.b = Bv[ic];
    if (!v) {
        L.a = v4i{0, 0, MT_RSEQ_NONE, 0};
        L.b = v4u{0u, 0u, 0u, 0u};
    }
    int ol = obs_len(L.a);
    if constexpr (kView) {
        u64 o = O[ic];
        if (!v) o = 0ull;
        bool ovl = ovl_has(o, V.cs);
        if (o & MT_OVF_BIT) ovl = loc_ovf_member(V.ovf, V.OA, o, V.c);
        const bool ins = (seg_cli(L.a) == V.c) | ((L.a.y != -1) & (L.a.y <= V.r));
        const bool gone = (L.a.z != MT_RSEQ_NONE) & ((seg_rcli(L.a) == V.c) | ovl | ((L.a.z != -1) & (L.a.z <= V.r)));
        const int vl = (ins & !gone) ? L.a.x : 0, pl = L.a.x * ((int)ins - (int)gone);
        nacc += V.local ? ol : pl;
        ol = V.local ? ol : vl;   // (from here on: the row's length in the view)
    }
    const int incl = wave_scan_incl(ol);
    L.p0 = pos + incl - ol;
    pos += bcast(incl, 63);
    L.vis = v & (ol > 0) & (L.p0 < Q.e) & (L.p0 + ol > Q.s);
    const bool marker = (L.b.z & MT_MARKER_BIT) != 0u;
    L.units = (L.vis & !marker & ((what & MT_WALK_TEXT) != 0u)) ? ol : 0;
    const uint32_t hi = L.b.y < P ? L.b.y : 0u;
    const uint32_t c = pr[(size_t)hi * MT_PREC];
    const bool ok = (hi != 0u) & (c <= (uint32_t)MT_KMAX);
    L.wc = (L.vis & ok & ((what & MT_WALK_PROPS) != 0u)) ? 1 + 2 * (int)c : 0;
    return L;
}
// query q's view: false with the mark when its refSeq lies outside the document's collab window
template <bool kView>
__device__ __forceinline__ bool walk_view(const DevState &st, int q, int doc, const WalkViewArgs<kView> &va, WalkView &V) {
    V.local = true;
    V.r = V.c = V.cs = V.OA = 0;
    V.ovf = nullptr;
    if constexpr (kView) {
        V.c = va.client[q];
        V.r = va.ref_seq[q];
        V.local = V.c == 0;
        if (V.local) return true;
        const DocHdr h = st.hdr[doc];
        if (V.r < h.min_seq || V.r > h.cur_seq) return false;
        const u64 sm = ballot(st.oslot[((size_t)doc * MT_OSLOTS + lane()) * 2] == V.c);
        V.cs = sm ? first_lane(sm) + 1 : 0;
        if (h.pad[HDR_PAGED]) {
            const PagedBase pb = doc_paged(st, doc);
            V.ovf = pb.ovf;
            V.OA = pb.OA;
        }
    }
    return true;
}
// A paged document's remote view from its unsettled-segment table (pg_store leaves it in HBM on
// every paged tier, HDR_UTN entries {page id, row stamps, overlap mask}; the growth step copies
// it): a row whose view length differs from its observer length is unsettled -- seq or
// removedSeq above minSeq -- so it has an entry, and an entry of a row that has settled since
// contributes 0 in every legal view (refSeq >= minSeq).  One pass, 64 entries at a time, gives
// the anomalous length sum len * (gone & !ins) (non-zero: N != L, the host answers) and adds
// each entry's vl - obs_len to diff[page id] (LDS).  Entries past the count read entry 0 and are
// masked; a page id outside the array is dropped (never seen: pg_load
// refuses such a document).
__device__ __forceinline__ int walk_table(const PagedBase &pb, int utn, const WalkView &V, int *diff) {
    for (int i = lane(); i < pb.PP; i += MT_WAVE) diff[i] = 0;
    __syncthreads();
    int anom = 0;
    for (int base = 0; base < utn; base += MT_WAVE) {
        const int e = base + lane();
        const bool v = e < utn;
        const int ec = v ? e : 0;
        const int pg = pb.upage[ec];
        v4i a = pb.uA[ec];
        u64 o = pb.uO[ec];
        if (!v) {
            a = v4i{0, 0, MT_RSEQ_NONE, 0};
            o = 0ull;
        }
        bool ovl = ovl_has(o, V.cs);
        if (o & MT_OVF_BIT) ovl = loc_ovf_member(V.ovf, V.OA, o, V.c);
        const bool ins = (seg_cli(a) == V.c) | ((a.y != -1) & (a.y <= V.r));
        const bool gone = (a.z != MT_RSEQ_NONE) & ((seg_rcli(a) == V.c) | ovl | ((a.z != -1) & (a.z <= V.r)));
        const int d = ((ins & !gone) ? a.x : 0) - obs_len(a);
        anom += (gone & !ins) ? a.x : 0;
        if (v && d != 0 && (uint32_t)pg < (uint32_t)pb.PP) atomicAdd(&diff[pg], d);
    }
    __syncthreads();
    return wave_sum(anom);
}
// walk_seek on the view's page lengths PageMeta.obs + diff[page id]
__device__ __forceinline__ void walk_seek_view(const SegRanges &R, const int *diff, int PP, int s, int &r0, int &pos,
                                               int &rows) {
    r0 = pos = rows = 0;
    bool at = false;
    for (int base = 0; !at && base < R.nr; base += MT_WAVE) {
        const int j = base + lane();
        const bool v = j < R.nr;
        const int pg = R.dir[v ? j : 0];
        const PageMeta pm = R.meta[pg];
        const int ob = v ? pm.obs + diff[(uint32_t)pg < (uint32_t)PP ? pg : 0] * ((uint32_t)pg < (uint32_t)PP) : 0, ns = v ? (int)pm.nseg : 0;
        const int oin = wave_scan_incl(ob), nin = wave_scan_incl(ns);
        const u64 m = ballot(v & (pos + oin > s));
        if (m) {
            const int l = first_lane(m);
            r0 = base + l;
            pos += bcast(oin - ob, l);
            rows += bcast(nin - ns, l);
            at = true;
        } else {
            pos += bcast(oin, 63);
            rows += bcast(nin, 63);
        }
    }
    if (!at) r0 = R.nr;
}
// A remote view of a flat document, of a paged one whose page capacity does not fit the LDS
// array, or under MT_LOCATE_ROW_WALK=1 walks every row from row 0 in the count pass (N and L
// are sums over the rows) and starts its gather at row 0.  A remote view of any other paged
// document decides N != L from the table, seeks its first page on the view's page lengths and
// stops at the end; the gather starts where the count pass did (va.seek).  The replica's own
// view walks as k_walk_count<false> does.
template <bool kView>
__global__ void __launch_bounds__(MT_WAVE) k_walk_count(DevState st, int nq, const uint32_t *docs, const int32_t *start,
                                                        const int32_t *end, uint32_t what, int skip, int64_t *n_rows,
                                                        int64_t *n_units, int64_t *n_words, int32_t *end_seen,
                                                        WalkViewArgs<kView> va) {
    extern __shared__ int s_diff[];
    const int q = blockIdx.x;
    if (q >= nq) return;
    const WalkQuery Q = walk_query(st, q, docs, start, end);
    WalkView V;
    const bool legal = walk_view<kView>(st, q, Q.doc, va, V);
    bool full = kView && !V.local;   // every row is read: N and L
    int rows_n = 0, units = 0, words = 0, pos = 0, nacc = 0, mark = legal ? 0 : MT_WALKQ_INVALID;
    if (legal && (Q.e > 0 || full)) {
        const DocHdr h = st.hdr[Q.doc];
        const SegRanges R = seg_ranges(st, Q.doc, h);
        const PagedBase ar = doc_paged(st, Q.doc);   // (the arenas of the document's region)
        const uint32_t P = (uint32_t)ar.P;
        const uint32_t *pr = ar.props + (size_t)h.props_half * P * MT_PREC;
        int r0 = 0, rows = 0;
        bool host = false;
        if constexpr (kView) {
            if (full && skip && R.paged && ar.PP <= va.lds_pages) {
                host = walk_table(ar, min(max(h.pad[HDR_UTN], 0), ar.UT), V, s_diff) != 0;
                full = false;
                mark = MT_WALKQ_SKIP;
                if (!host) walk_seek_view(R, s_diff, ar.PP, Q.s, r0, pos, rows);
                if (lane() == 0) {
                    va.seek[3 * q] = r0;
                    va.seek[3 * q + 1] = pos;
                    va.seek[3 * q + 2] = rows;
                }
            }
        }
        if (mark != MT_WALKQ_SKIP) walk_seek(R, Q.s, full ? 0 : skip, r0, pos, rows);
        for (int r = r0; !host && r < R.count() && (full || pos < Q.e); r++) {
            const v4i *A;
            const v4u *Bv;
            int n;
            R.get(r, A, Bv, n);
            const u64 *O = R.O + (A - R.A);
            for (int base = 0; base < n && (full || pos < Q.e); base += MT_WAVE) {
                const WalkLane L = walk_chunk<kView>(A, O, Bv, base + lane(), n, Q, V, what, pr, P, pos, nacc);
                rows_n += __popcll(ballot(L.vis));
                units += L.units;
                words += L.wc;
            }
        }
        units = wave_sum(units);
        words = wave_sum(words);
        if (host || (full && wave_sum(nacc) != pos)) {   // N != L: the host answers, counts included
            mark = MT_WALKQ_HOST;
            rows_n = units = words = 0;
        }
    }
    if (lane() == 0) {
        n_rows[q] = rows_n;
        n_units[q] = units;
        n_words[q] = words;
        end_seen[q] = Q.open ? pos : Q.e;   // (an open walk ran to the document's end: pos is its length)
        if constexpr (kView) va.mark[q] = mark;
    }
}
// Writes query q's records at rows[row_off[q] ..), its texts at text[text_off[q] ..) and its
// property records at records[word_off[q] ..).  Per chunk a visited lane writes its own record at
// the rows done plus its rank in the ballot, and copies its property record (<= 17 words, a
// per-lane loop, as k_props_gather) to the words done plus an exclusive scan of the chunk's word
// counts.  The texts are copied as k_text_gather<false> copies clipped ones: the chunk's
// destination offsets (a wave scan) and sources in LDS, the chunk's output units dealt across the
// lanes in 4-byte destination words, the odd head, the tail and the carry between chunks stored
// as single units.  (The dealing is written again here and not shared with k_text_gather: there
// the clip, the marker unit and the per-segment A/B variant are woven into it, and a shared
// helper would recompile a kernel whose timing is recorded.)  Rows, units and words are checked
// against the query's three slots: the state cannot change between the passes, but a wrong count
// must not become a store outside the result.
template <bool kView>
__global__ void __launch_bounds__(MT_WAVE) k_walk_gather(DevState st, int nq, const uint32_t *docs,
                                                         const int32_t *start, const int32_t *end, uint32_t what,
                                                         int skip, const int32_t *end_seen, const int64_t *row_off,
                                                         const int64_t *text_off, const int64_t *word_off,
                                                         mt_walk_row *rows_out, uint16_t *text_out,
                                                         uint32_t *records, WalkViewArgs<kView> va) {
    __shared__ int s_dst[MT_WAVE], s_src[MT_WAVE];
    const int q = blockIdx.x;
    if (q >= nq) return;
    WalkQuery Q = walk_query(st, q, docs, start, end);
    WalkView V;
    bool took = false;   // the count pass started at a page the table-based seek found
    if constexpr (kView) {
        const int mk = va.mark[q];
        if (mk & (MT_WALKQ_HOST | MT_WALKQ_INVALID)) return;   // (the host writes a marked query's slots)
        took = mk == MT_WALKQ_SKIP;
    }
    walk_view<kView>(st, q, Q.doc, va, V);
    int nacc = 0;
    const int64_t room_r = row_off[q + 1] - row_off[q], room_t = text_off[q + 1] - text_off[q],
                  room_w = word_off[q + 1] - word_off[q];
    if (Q.e <= 0 || room_r <= 0) return;
    const int E = end_seen[q];   // the leaf action's end: an undefined one resolved by the count pass
    const DocHdr h = st.hdr[Q.doc];
    const SegRanges R = seg_ranges(st, Q.doc, h);
    const PagedBase ar = doc_paged(st, Q.doc);   // (the arenas of the document's region)
    const uint32_t P = (uint32_t)ar.P, T = (uint32_t)ar.T;
    const uint32_t *pr = ar.props + (size_t)h.props_half * P * MT_PREC;
    const uint16_t *tb = ar.text + (size_t)h.text_half * ar.T;
    mt_walk_row *rw = rows_out + row_off[q];
    uint32_t *rec = records + word_off[q];
    uint16_t *o = text_out + text_off[q];
    const int odd = (int)(((uintptr_t)o >> 1) & 1);   // the slot starts on the second half of a word
    // unit u of the chunk (units of row sg start at s_dst[sg])
    auto unit_at = [&](int u) -> uint32_t {
        int sg = 0;
#pragma unroll
        for (int step = MT_WAVE / 2; step > 0; step >>= 1)
            if (s_dst[sg + step] <= u) sg += step;
        const uint32_t ix = (uint32_t)s_src[sg] + (uint32_t)(u - s_dst[sg]);
        return ix < T ? tb[ix] : 0u;
    };
    int r0, pos, rows;
    walk_seek(R, Q.s, kView && !V.local ? 0 : skip, r0, pos, rows);
    if constexpr (kView) {
        if (took) {
            r0 = min(max(va.seek[3 * q], 0), R.count());
            pos = va.seek[3 * q + 1];
            rows = va.seek[3 * q + 2];
        }
    }
    int64_t rows_done = 0, words_done = 0;
    int64_t done = 0;        // units of the query produced so far (the carried one included)
    bool carry = false;      // unit done - 1 is the first half of a word not yet stored
    uint32_t carry_v = 0;
    for (int r = r0; r < R.count() && pos < Q.e; r++) {
        const v4i *A;
        const v4u *Bv;
        int n;
        R.get(r, A, Bv, n);
        const u64 *O = R.O + (A - R.A);
        for (int base = 0; base < n && pos < Q.e; base += MT_WAVE) {
            const WalkLane L = walk_chunk<kView>(A, O, Bv, base + lane(), n, Q, V, what, pr, P, pos, nacc);
            const u64 vm = ballot(L.vis);
            if (!vm) continue;
            const int incl = wave_scan_incl(L.units), winc = wave_scan_incl(L.wc);
            const int64_t rank = rows_done + __popcll(vm & ((1ull << lane()) - 1ull));
            const int64_t w0 = words_done + winc - L.wc, t0 = done + incl - L.units;
            const bool wfits = (L.wc > 0) & (w0 + L.wc <= room_w);
            const bool tfits = (L.units > 0) & (t0 + L.units <= room_t);
            if (L.vis && rank < room_r) {
                const bool marker = (L.b.z & MT_MARKER_BIT) != 0u;
                mt_walk_row w;
                w.row = rows + base + lane();
                w.uid = L.b.z & ~MT_MARKER_BIT;
                w.position = L.p0;
                w.length = L.a.x;
                w.seq = L.a.y >= MT_LOCAL_BASE ? -1 : L.a.y;
                w.client = (int)(short)(L.a.w & 0xFFFF);
                w.marker_ref_type = marker ? (int32_t)L.b.x : -1;
                w.text = tfits ? (uint32_t)t0 : MT_PROPS_NONE;
                w.props = wfits ? (uint32_t)w0 : MT_PROPS_NONE;
                w.start = Q.s - L.p0;
                w.end = E - L.p0;
                w.flags = 0u;
                rw[rank] = w;
            }
            if (wfits) {
                const uint32_t *x = pr + (size_t)L.b.y * MT_PREC;   // (wc > 0: the handle is inside the arena)
                rec[w0] = (uint32_t)(L.wc >> 1);
                for (int k = 1; k < L.wc; k++) rec[w0 + k] = x[k];
            }
            rows_done += __popcll(vm);
            words_done += bcast(winc, 63);
            int tot = bcast(incl, 63);
            // (the unit guard is apart from tfits on purpose: were a count ever wrong, a row cut by
            // the room would have units stored and a text field of "nothing" -- never a stray store)
            if (done + tot > room_t) tot = (int)(room_t - done);
            if (tot <= 0) continue;
            __syncthreads();   // the previous chunk's readers are done with the LDS arrays
            s_dst[lane()] = incl - L.units;
            s_src[lane()] = (int)L.b.x;
            __syncthreads();
            // chunk-local unit u lies at o[done + u]; u = -1 is the carried unit
            int u0 = carry ? -1 : 0;
            if (!carry && ((done + odd) & 1)) {   // the query's odd head (done == 0 here)
                if (lane() == 0) o[done] = (uint16_t)unit_at(0);
                u0 = 1;
            }
            const int npair = (tot - u0) >> 1;
            for (int k = lane(); k < npair; k += MT_WAVE) {
                const int u = u0 + 2 * k;
                const uint32_t a = u < 0 ? carry_v : unit_at(u), b = unit_at(u + 1);
                *(uint32_t *)(o + done + u) = a | (b << 16);
            }
            carry = ((tot - u0) & 1) != 0;
            if (carry) carry_v = unit_at(tot - 1);
            done += tot;
        }
        rows += n;
    }
    if (carry && lane() == 0) o[done - 1] = (uint16_t)carry_v;   // the tail
}

// ---------------------------------------------------------------- bulk delta-log read-out
// mt_get_delta_log for many (doc, from_word) queries, and the rows of mt_delta_range: one wave
// per query.  A query's span is its document's log from from_word to the word count (clamped
// into [0, DL] as mt_get_delta_log clamps it), so nothing outside the document's own log is
// read.  The records are variable-length and each header tells where the next one starts, so
// the walk (mt_dlog.h) is serial per query: every lane of the wave runs it on the same
// wave-uniform addresses (one cache line per load, no divergence) and lane 0 stores the rows;
// the queries are the parallelism.
static_assert(sizeof(mt_delta_range) == 32, "mt_delta_range size");
struct DlogSpan {
    const int32_t *src;
    int words;
    uint32_t flags;
};
__device__ __forceinline__ DlogSpan dlog_span(const DevState &st, int q, const uint32_t *docs, const int32_t *from) {
    // (the host refuses doc >= n_docs and from_word < 0; a query that held one anyway reads nothing)
    const uint32_t dq = docs ? docs[q] : (uint32_t)q;
    const bool known = dq < (uint32_t)st.n_docs;
    const uint32_t doc = known ? dq : 0u;
    const int f = max(from ? from[q] : 0, 0);
    const int have = known ? min(max(st.hdr[doc].dlog_n, 0), st.DL) : 0;
    DlogSpan s;
    s.flags = st.hdr[doc].pad[HDR_DLOG_OVF] ? MT_DLOG_OVERFLOWED : 0u;
    if (f > have) s.flags |= MT_DLOG_PAST;
    s.words = f > have ? 0 : have - f;
    s.src = st.dlog + (size_t)doc * st.DL + min(f, have);
    return s;
}
__global__ void __launch_bounds__(MT_WAVE) k_dlog_count(DevState st, int nq, const uint32_t *docs, const int32_t *from,
                                                        int want_rows, int64_t *n_words, int64_t *n_rows,
                                                        uint32_t *flags) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    DlogSpan s = dlog_span(st, q, docs, from);
    int64_t rows = 0;
    if (want_rows && s.words > 0) {
        mt_dlog_count c;
        if (mt_dlog_walk(s.src, s.words, st.DLR != 0, c))
            rows = c.n;
        else
            s.flags |= MT_DLOG_BAD;
    }
    if (lane() == 0) {
        n_words[q] = s.words;
        if (want_rows) n_rows[q] = rows;
        flags[q] = s.flags;
    }
}
// n words from src to dst, V words per access in the body: the caller picks the widest V at
// which src and dst are congruent, the head runs to dst's first V-word boundary (so src's too)
// and the tail takes what is left; both are shorter than V words.
template <int V> __device__ __forceinline__ void dlog_copy(int32_t *dst, const int32_t *src, int n) {
    typedef int32_t vec __attribute__((ext_vector_type(V)));
    const int head = min(n, (int)((V - (int)(((uintptr_t)dst >> 2) % V)) % V));
    if (lane() < head) dst[lane()] = src[lane()];
    const int nv = (n - head) / V;
    const vec *s = (const vec *)(src + head);
    vec *d = (vec *)(dst + head);
    for (int i = lane(); i < nv; i += MT_WAVE) d[i] = s[i];
    const int done = head + nv * V;
    if (lane() < n - done) dst[done + lane()] = src[done + lane()];
}
struct DlogFill {   // the walk's sink of the fill pass: lane 0 stores, rows beyond the query's slots are dropped
    mt_delta_range *rows;
    int64_t room, n;
    int q;
    __device__ void entry(const mt_dlog_entry &e) {
        if (n < room && lane() == 0)
            rows[n] = mt_delta_range{q, e.record, e.seq, e.kind, e.position, e.length, e.word, e.uid};
        n++;
    }
};
// Writes query q's words at out[off[q] ..) and, with row_off, its rows at rows[row_off[q] ..).
// Words and rows are checked against the query's slots.  A span that is not well formed was
// given no slot by the counting pass and is not walked again.
__global__ void __launch_bounds__(MT_WAVE) k_dlog_gather(DevState st, int nq, const uint32_t *docs, const int32_t *from,
                                                         const int64_t *off, const int64_t *row_off, int32_t *out,
                                                         mt_delta_range *rows) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const DlogSpan s = dlog_span(st, q, docs, from);
    const int n = (int)min((int64_t)s.words, off[q + 1] - off[q]);
    if (n <= 0) return;
    int32_t *dst = out + off[q];
    const uint32_t rel = (uint32_t)((uintptr_t)s.src - (uintptr_t)dst);
    if ((rel & 15u) == 0u)
        dlog_copy<4>(dst, s.src, n);
    else if ((rel & 7u) == 0u)
        dlog_copy<2>(dst, s.src, n);
    else
        for (int i = lane(); i < n; i += MT_WAVE) dst[i] = s.src[i];
    if (!row_off) return;
    DlogFill f{rows + row_off[q], row_off[q + 1] - row_off[q], 0, q};
    if (f.room > 0) mt_dlog_walk(s.src, s.words, st.DLR != 0, f);
}
// mt_delta_log_reset for the listed documents
__global__ void __launch_bounds__(MT_WAVE) k_dlog_reset_docs(DevState st, int n, const uint32_t *docs) {
    const int i = blockIdx.x * MT_WAVE + threadIdx.x;
    if (i >= n) return;
    const uint32_t doc = docs ? docs[i] : (uint32_t)i;
    if (doc >= (uint32_t)st.n_docs) return;
    st.hdr[doc].dlog_n = 0;
    st.hdr[doc].pad[HDR_DLOG_OVF] = 0;
}

// ---------------------------------------------------------------- bulk segment read-outs
// MergeTree.getContainingSegment / getPosition / getLength (MT/mergeTree.ts:1610-1667) for many
// (doc, pos | uid, refSeq, client) queries: one wave per query over the document's rows in
// chunks of 64, as k_text_count walks.  In a view (c, r) a row is inserted (ins) and removed
// (gone) by view_len's two tests, with the overflow set read when the mask carries MT_OVF_BIT
// (ovf_member, host_view_vis).  One walk sums
//     N = sum len * (ins - gone)   -- the root's partial length, getLength in the view
//     L = sum view_len             -- the leaves' lengths
// N = L - (the lengths of the rows with gone and not ins), so N == L exactly when no row of
// positive length is removed but not inserted in the view; every interior partial length is
// then the sum of its leaves' view lengths, all of them >= 0, and searchBlock's descent (the
// first child whose length exceeds pos, at every level) ends at the first row whose inclusive
// view_len prefix exceeds pos -- or at none when pos >= L -- and getPosition is the exclusive
// prefix.  Otherwise the query is marked for the host path.
// Observer view (c == 0): N == L always; the walk stops at the answer's chunk and, on a paged
// document, finds the page by the directory's PageMeta.obs prefix sums (by position) or by the
// uid map (a hint: the page must be in the directory and hold the uid, else the rows are
// walked) and reads that page's rows only.
#define MT_LOC_HOST 1      // aux mark: a view with N != L, answered on the host
#define MT_LOC_INVALID 2   // aux mark: a remote refSeq outside [minSeq, currentSeq]
static_assert(sizeof(mt_seg_hit) == 48, "mt_seg_hit size");
struct LocWalk {           // wave-uniform
    int vpos, opos, rows;  // view / observer length and rows before the current range
    int nacc;              // (per lane) its rows' terms of N
    bool found;
    mt_seg_hit hit;
};
__device__ static bool loc_ovf_member(const uint16_t *ovf, int OA, u64 o, int c) {
    const uint32_t off = (uint32_t)o;
    if (!ovf || off >= (uint32_t)OA) return false;
    const uint32_t n = ovf[off];
    bool in = false;
    for (uint32_t k = 1; k <= n && off + k < (uint32_t)OA; k++) in = in | (ovf[off + k] == (uint16_t)c);
    return in;
}
// rows [base, base + 64) of a range of n rows (kMode 0: locate position key, 1: locate uid key,
// 2: lengths only)
template <int kMode>
__device__ __forceinline__ void loc_chunk(LocWalk &W, const v4i *A, const u64 *O, const v4u *Bv, int base, int n, int key,
                                          bool local, int r, int c, int cs, const uint16_t *ovf, int OA) {
    const int i = base + lane();
    const bool v = i < n;
    const int ic = v ? i : 0;
    v4i a = A[ic];
    u64 o = O[ic];   // (unconditional: DESIGN section 10)
    v4u b = v4u{0u, 0u, 0u, 0u};
    if (kMode != 2) b = Bv[ic];
    if (!v) {
        a = v4i{0, 0, MT_RSEQ_NONE, 0};
        o = 0ull;
    }
    const int ol = obs_len(a);
    int vl = ol, pl = ol;
    if (!local) {
        bool ovl = ovl_has(o, cs);
        if (o & MT_OVF_BIT) ovl = loc_ovf_member(ovf, OA, o, c);
        const bool ins = (seg_cli(a) == c) | ((a.y != -1) & (a.y <= r));
        const bool gone = (a.z != MT_RSEQ_NONE) & ((seg_rcli(a) == c) | ovl | ((a.z != -1) & (a.z <= r)));
        vl = (ins & !gone) ? a.x : 0;
        pl = a.x * ((int)ins - (int)gone);
    }
    W.nacc += pl;
    const int vin = wave_scan_incl(vl);
    const int oin = local ? vin : wave_scan_incl(ol);
    if (kMode != 2 && !W.found) {
        const u64 m = kMode == 0 ? ballot(v & (W.vpos + vin > key)) : ballot(v & ((b.z & ~MT_MARKER_BIT) == (uint32_t)key));
        if (m) {
            const int l = first_lane(m);
            const int x = bcast(a.x, l), y = bcast(a.y, l), z = bcast(a.z, l), w = bcast(a.w, l);
            const uint32_t bx = (uint32_t)bcast((int)b.x, l), bz = (uint32_t)bcast((int)b.z, l);
            W.found = true;
            W.hit.row = W.rows + base + l;
            W.hit.uid = bz & ~MT_MARKER_BIT;
            W.hit.position = W.vpos + bcast(vin - vl, l);
            W.hit.offset = kMode == 0 ? key - W.hit.position : 0;
            W.hit.local_position = W.opos + bcast(oin - ol, l);
            W.hit.length = x;
            W.hit.seq = y >= MT_LOCAL_BASE ? -1 : y;
            W.hit.client = (int)(short)(w & 0xFFFF);
            W.hit.removed_seq = z >= MT_LOCAL_BASE ? -1 : z;
            W.hit.removed_client = z == MT_RSEQ_NONE ? MT_RSEQ_NONE : (int)(short)((uint32_t)w >> 16);
            W.hit.marker_ref_type = (bz & MT_MARKER_BIT) ? (int32_t)bx : -1;
        }
    }
    W.vpos += bcast(vin, 63);
    W.opos += bcast(oin, 63);
}
template <int kMode>
__global__ void __launch_bounds__(MT_WAVE) k_locate(DevState st, int nq, const uint32_t *docs, const int32_t *key,
                                                    const int32_t *ref_seq, const int32_t *client, int skip,
                                                    mt_seg_hit *out, v4i *aux) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int doc = docs ? (int)docs[q] : q;
    const int c = client ? client[q] : 0;
    const int r = ref_seq ? ref_seq[q] : 0;
    const int k = kMode == 2 ? 0 : key[q];
    const bool local = c == 0;
    LocWalk W;
    memset(&W.hit, 0, sizeof(W.hit));
    W.hit.row = -1;
    W.vpos = W.opos = W.rows = W.nacc = 0;
    W.found = false;
    int mark = 0, N = 0;
    if (doc < 0 || doc >= st.n_docs) {   // (the host refuses these)
        mark = MT_LOC_INVALID;
    } else {
        const DocHdr h = st.hdr[doc];
        if (!local && (r < h.min_seq || r > h.cur_seq)) {
            mark = MT_LOC_INVALID;
        } else {
            const u64 sm = ballot(st.oslot[((size_t)doc * MT_OSLOTS + lane()) * 2] == c);
            const int cs = !local && sm ? first_lane(sm) + 1 : 0;
            const SegRanges R = seg_ranges(st, doc, h);
            const uint16_t *ovf = nullptr, *umap = nullptr;
            int OA = 0, UM = 0, PP = 0;
            if (R.paged) {
                const PagedBase pb = doc_paged(st, doc);
                ovf = pb.ovf;
                OA = pb.OA;
                umap = pb.umap;
                UM = pb.UM;
                PP = pb.PP;
            }
            bool walk = true;
            if (local && R.paged && skip) {
                // the page by the directory (64 positions at a time); by uid: the page the map names
                int target = -1;
                if (kMode == 1 && (uint32_t)k < (uint32_t)UM) target = umap[(uint32_t)k];
                if (target >= PP) target = -1;
                walk = kMode == 1 && target < 0;
                bool at = false;
                for (int base = 0; !walk && !at && base < R.nr; base += MT_WAVE) {
                    const int j = base + lane();
                    const bool v = j < R.nr;
                    const int pg = R.dir[v ? j : 0];
                    const PageMeta pm = R.meta[pg];
                    const int ob = v ? pm.obs : 0, ns = v ? (int)pm.nseg : 0;
                    const int oin = wave_scan_incl(ob), nin = wave_scan_incl(ns);
                    const u64 m = kMode == 0 ? ballot(v & (W.opos + oin > k)) : (kMode == 1 ? ballot(v & (pg == target)) : 0ull);
                    if (m) {
                        const int l = first_lane(m);
                        const size_t p0 = (size_t)bcast(pg, l) * MT_PG_SLOTS;
                        W.opos += bcast(oin - ob, l);
                        W.rows += bcast(nin - ns, l);
                        W.vpos = W.opos;
                        loc_chunk<kMode>(W, R.A + p0, R.O + p0, R.B + p0, 0, min(bcast(ns, l), MT_PG_SLOTS), k, true, r, c, 0,
                                         ovf, OA);
                        at = true;
                    } else {
                        W.opos += bcast(oin, 63);
                        W.rows += bcast(nin, 63);
                        W.vpos = W.opos;
                    }
                }
                // no page holds it: past the end by position (the directory's total is the length);
                // by uid the map was stale or the page not the segment's: walk the rows
                if (kMode == 1 && !W.found) walk = true;
                if (kMode == 0 && at && !W.found) walk = true;   // (obs and the page's rows disagree: never seen)
                if (walk) W.vpos = W.opos = W.rows = W.nacc = 0;
            }
            if (walk) {
                for (int rr = 0; rr < R.count() && !(local && W.found); rr++) {
                    const v4i *A;
                    const v4u *Bv;
                    int n;
                    R.get(rr, A, Bv, n);
                    const u64 *O = R.O + (A - R.A);
                    for (int base = 0; base < n && !(local && W.found); base += MT_WAVE)
                        loc_chunk<kMode>(W, A, O, Bv, base, n, k, local, r, c, cs, ovf, OA);
                    W.rows += n;
                }
            }
            // (observer view: N == L; the sum is whole only when the walk did not stop at a hit)
            N = local ? W.vpos : wave_sum(W.nacc);
            if (kMode != 2 && N != W.vpos) mark = MT_LOC_HOST;
        }
    }
    if (lane() == 0) {
        if (kMode != 2) out[q] = W.hit;
        aux[q] = v4i{mark, N, W.opos, 0};
    }
}

// ---------------------------------------------------------------- bulk marker queries
// MergeTree.findTile (MT/mergeTree.ts:1796-1822) and getMarkerFromId (:1965) for many queries in
// the observer view: one wave per query, one lane per row in chunks of 64.
// A row qualifies for a label when it is a marker with the Tile bit whose property record holds
// the tile key with a value of the label's set (refHasTileLabel, :620-635); by id, when it is a
// marker whose record holds the id key with the id's value.  With H the first row whose
// inclusive observer prefix exceeds pos:
//   preceding (search + tileShift, :1030-1069, :1830-1862): the last qualifying visible row at or
//     before H; no H (pos >= length, or pos < 0: undefined): the last one of the document;
//   following (backwardSearch, :1864-1907): the first qualifying visible row at or after H;
//     pos < 0: the first one of the document; pos == length: the last row, removed or not, when
//     it qualifies; pos > length: nothing.
// Interior blocks answer from rightmostTiles / leftmostTiles, which hold rows of positive
// localNetLength only (:262-317): hence "visible".
struct TileQuery {         // wave-uniform
    uint32_t key;          // the tile key (mode 0) / the id key (mode 1)
    const uint32_t *vals;  // mode 0: the label's value ids, ascending
    int nvals;
    uint32_t id;           // mode 1: the id's value id
    const uint32_t *pr;    // the document's property records
    uint32_t P;
};
struct TileWalk {          // wave-uniform
    int opos, rows;        // observer length and rows before the current chunk
    int examined;          // rows tested
    bool hfound, found, dup;
    mt_seg_hit hit;
};
// the row test of one lane: its row (a, b) is a valid one of the chunk
template <int kMode> __device__ __forceinline__ bool tile_row_test(const TileQuery &Q, bool v, v4u b) {
    const bool mk = v & ((b.z & MT_MARKER_BIT) != 0u);
    // a handle outside the arena or a count over MT_KMAX reads as no record; the words are
    // loaded unconditionally (record 0 for the other lanes) and masked
    const uint32_t hi = (mk & (b.y < Q.P)) ? b.y : 0u;
    const uint32_t *rec = Q.pr + (size_t)hi * MT_PREC;
    const uint32_t c = rec[0];
    const bool ok = (hi != 0u) & (c <= (uint32_t)MT_KMAX);
    uint32_t tv = MT_VAL_NULL;   // the key's value (one pair per key)
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)MT_KMAX; k++) {
        const uint32_t kk = rec[1 + 2 * k], vv = rec[2 + 2 * k];
        tv = ((k < c) & (kk == Q.key)) ? vv : tv;
    }
    const bool has = ok & (tv < MT_VAL_UNDEF);
    const uint32_t mv = tv & ~(MT_VAL_FALSY_BIT | MT_VAL_NOMATCH_BIT);
    if (kMode == 1) return has & (mv == Q.id);
    bool in = false;
    for (int j = 0; j < Q.nvals; j++) in = in | (Q.vals[j] == mv);   // (a handful of ids; the span is wave-uniform)
    return has & in & ((b.x & 1u) != 0u);
}
__device__ __forceinline__ void tile_fill(TileWalk &W, int l, int base, v4i a, v4u b, int excl) {
    const int x = bcast(a.x, l), y = bcast(a.y, l), z = bcast(a.z, l), w = bcast(a.w, l);
    const uint32_t bx = (uint32_t)bcast((int)b.x, l), bz = (uint32_t)bcast((int)b.z, l);
    W.found = true;
    W.hit.row = W.rows + base + l;
    W.hit.uid = bz & ~MT_MARKER_BIT;
    W.hit.position = W.hit.local_position = W.opos + bcast(excl, l);
    W.hit.offset = 0;
    W.hit.length = x;
    W.hit.seq = y >= MT_LOCAL_BASE ? -1 : y;
    W.hit.client = (int)(short)(w & 0xFFFF);
    W.hit.removed_seq = z >= MT_LOCAL_BASE ? -1 : z;
    W.hit.removed_client = z == MT_RSEQ_NONE ? MT_RSEQ_NONE : (int)(short)((uint32_t)w >> 16);
    W.hit.marker_ref_type = (bz & MT_MARKER_BIT) ? (int32_t)bx : -1;
}
// rows [base, base + 64) of a range of n rows.  kMode 0: until H is known (W.hfound) the chunk
// is searched for it; preceding takes the highest qualifying visible lane at or below H (any
// lane while there is no H), following the lowest one at or above H (none before H).  kMode 1:
// the first matching lane, then any further match marks a duplicate.  last: the pos == length
// edge -- lane n - 1 - base answers if it qualifies, whatever its length.
template <int kMode>
__device__ __forceinline__ void tile_chunk(TileWalk &W, const TileQuery &Q, const v4i *A, const v4u *Bv, int base, int n,
                                           int pos, bool prec, bool last) {
    const int i = base + lane();
    const bool v = i < n;
    const int ic = v ? i : 0;
    v4i a = A[ic];   // (unconditional: DESIGN section 10)
    v4u b = Bv[ic];
    if (!v) {
        a = v4i{0, 0, MT_RSEQ_NONE, 0};
        b = v4u{0u, 0u, 0u, 0u};
    }
    const int ol = obs_len(a);
    const int oin = wave_scan_incl(ol);
    const bool q = tile_row_test<kMode>(Q, v, b);
    W.examined += min(n - base, MT_WAVE);
    if (kMode == 1) {
        const u64 m = ballot(q);
        if (m) {
            W.dup = W.dup | W.found | ((m & (m - 1)) != 0ull);
            if (!W.found) tile_fill(W, first_lane(m), base, a, b, oin - ol);
        }
    } else if (last) {
        const int l = n - 1 - base;
        if ((ballot(q) >> l) & 1ull) tile_fill(W, l, base, a, b, oin - ol);
    } else {
        u64 lanes = ~0ull;
        if (!W.hfound && pos >= 0) {
            const u64 mh = ballot(v & (W.opos + oin > pos));
            if (mh) {
                const int lh = first_lane(mh);
                W.hfound = true;
                lanes = prec ? (~0ull >> (63 - lh)) : (~0ull << lh);
            } else if (!prec) {
                lanes = 0ull;
            }
        }
        const u64 cand = ballot(q & (ol > 0)) & lanes;
        if (cand) tile_fill(W, prec ? 63 - __clzll((long long)cand) : first_lane(cand), base, a, b, oin - ol);
    }
    W.opos += bcast(oin, 63);
}
template <int kMode>
__global__ void __launch_bounds__(MT_WAVE) k_tiles(DevState st, int nq, const uint32_t *docs, const int32_t *posv,
                                                   const uint32_t *sel, uint32_t key, const uint32_t *label_off,
                                                   const uint32_t *label_vals, int skip, mt_seg_hit *out,
                                                   int32_t *examined) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int doc = docs ? (int)docs[q] : q;
    // mode 0: sel = label index | preceding << 31; mode 1: sel = the id's value id
    const uint32_t s = sel[q];
    const int pos = kMode == 0 ? posv[q] : -1;
    const bool prec = kMode == 0 && (s >> 31) != 0u;
    TileWalk W;
    memset(&W.hit, 0, sizeof(W.hit));
    W.hit.row = -1;
    W.opos = W.rows = W.examined = 0;
    W.hfound = W.found = W.dup = false;
    if (doc >= 0 && doc < st.n_docs) {   // (the host refuses the others)
        const DocHdr h = st.hdr[doc];
        const SegRanges R = seg_ranges(st, doc, h);
        const PagedBase ar = doc_paged(st, doc);   // (the arenas of the document's region)
        TileQuery Q;
        Q.key = key;
        Q.P = (uint32_t)ar.P;
        Q.pr = ar.props + (size_t)h.props_half * ar.P * MT_PREC;
        Q.id = s;
        Q.vals = label_vals;
        Q.nvals = 0;
        if (kMode == 0) {
            const uint32_t l = s & 0x7FFFFFFFu, lo = label_off[l];
            Q.vals = label_vals + lo;
            Q.nvals = (int)(label_off[l + 1] - lo);
        }
        bool walk = true;
        int total = -1;   // the observer length, once the directory has given it
        if (kMode == 0 && R.paged && skip && R.nr > 0) {
            const int PP = ar.PP;
            auto page_of = [&](int j) {   // (a directory entry outside the region reads as page 0)
                const int pg = R.dir[j];
                return pg < PP ? pg : 0;
            };
            // H's page by the directory's observer lengths, 64 positions at a time; following
            // with pos undefined starts at the first page and needs no scan
            int hp = -1, nrows = 0;
            if (prec || pos >= 0) {
                for (int base = 0; hp < 0 && base < R.nr; base += MT_WAVE) {
                    const int j = base + lane();
                    const bool v = j < R.nr;
                    const PageMeta pm = R.meta[page_of(v ? j : 0)];
                    const int ob = v ? pm.obs : 0, ns = v ? min((int)pm.nseg, MT_PG_SLOTS) : 0;
                    const int oin = wave_scan_incl(ob), nin = wave_scan_incl(ns);
                    const u64 m = pos >= 0 ? ballot(v & (W.opos + oin > pos)) : 0ull;
                    if (m) {
                        const int l = first_lane(m);
                        hp = base + l;
                        W.opos += bcast(oin - ob, l);
                        nrows += bcast(nin - ns, l);
                    } else {
                        W.opos += bcast(oin, 63);
                        nrows += bcast(nin, 63);
                    }
                }
            } else {
                hp = 0;
                W.hfound = true;   // every row of the document is at or after H
            }
            walk = false;
            if (hp < 0) {   // no H: W.opos is the document's length, nrows its rows
                total = W.opos;
                const PageMeta pm = R.meta[page_of(R.nr - 1)];
                const int ns = min((int)pm.nseg, MT_PG_SLOTS);
                const size_t p0 = (size_t)page_of(R.nr - 1) * MT_PG_SLOTS;
                W.opos -= pm.obs;
                W.rows = nrows - ns;
                if (prec) {
                    hp = R.nr - 1;   // the last qualifying visible row of the document: from the end
                } else if (pos == total && ns > 0) {
                    tile_chunk<kMode>(W, Q, R.A + p0, R.B + p0, 0, ns, pos, prec, true);
                }
            } else {
                W.rows = nrows;
            }
            // H's page (or the end the walk starts from), then away from it one page at a time
            const bool had_h = hp >= 0 && total < 0 && pos >= 0;
            for (int j = hp; hp >= 0 && j >= 0 && j < R.nr && !W.found; j += prec ? -1 : 1) {
                const int pg = page_of(j);
                const PageMeta pm = R.meta[pg];
                const int ns = min((int)pm.nseg, MT_PG_SLOTS);
                const size_t p0 = (size_t)pg * MT_PG_SLOTS;
                if (j < hp) {
                    W.opos -= pm.obs;
                    W.rows -= ns;
                }
                const int before = W.opos;
                tile_chunk<kMode>(W, Q, R.A + p0, R.B + p0, 0, ns, pos, prec, false);
                if (j == hp && had_h && !W.hfound) {   // (obs and the page's rows disagree: never seen)
                    walk = true;
                    break;
                }
                W.hfound = true;
                if (prec)
                    W.opos = before;
                else
                    W.rows += ns;
            }
            if (walk) {
                memset(&W.hit, 0, sizeof(W.hit));
                W.hit.row = -1;
                W.opos = W.rows = 0;
                W.hfound = W.found = false;
                total = -1;
            }
        }
        if (walk) {
            // from row 0: flat documents, by id, MT_LOCATE_ROW_WALK.  preceding stops at H's
            // chunk, following at the first answer; by id every row is read
            if (kMode == 0 && !prec && pos < 0) W.hfound = true;
            int n_last = 0;
            const v4i *A_last = nullptr;
            const v4u *B_last = nullptr;
            for (int rr = 0; rr < R.count(); rr++) {
                if (kMode == 0 && (prec ? W.hfound : W.found)) break;
                const v4i *A;
                const v4u *Bv;
                int n;
                R.get(rr, A, Bv, n);
                if (R.paged) n = min(n, MT_PG_SLOTS);
                for (int base = 0; base < n; base += MT_WAVE) {
                    if (kMode == 0 && (prec ? W.hfound : W.found)) break;
                    tile_chunk<kMode>(W, Q, A, Bv, base, n, pos, prec, false);
                }
                W.rows += n;
                n_last = n;   // (the last page, rows or none: the descent takes the last child)
                A_last = A;
                B_last = Bv;
            }
            // following, pos == length: no H was found and the whole document was walked
            if (kMode == 0 && !prec && !W.hfound && pos == W.opos && n_last > 0) {
                const int base = ((n_last - 1) / MT_WAVE) * MT_WAVE;
                W.rows -= n_last;
                // (the chunk's rows before the last one add up to length - its own: opos before it)
                int before = 0;
                {
                    const int i = base + lane();
                    const v4i a = A_last[i < n_last ? i : 0];
                    before = wave_sum(i < n_last ? obs_len(a) : 0);
                }
                W.opos -= before;
                tile_chunk<kMode>(W, Q, A_last, B_last, base, n_last, pos, prec, true);
            }
        }
    }
    if (lane() == 0) {
        W.hit.flags = W.dup ? MT_MARK_DUP : 0u;
        out[q] = W.hit;
        examined[q] = W.examined;
    }
}

// ============================================================================ host side
// ---------------------------------------------------------------- live-client reconnect
// regeneratePendingOp for the oldest pending segment group of one document (one wave):
// resetPendingDeltaToOps (MT/client.ts:709-766) with findReconnectionPostition (:675-707) --
// a segment counts towards the positions when it is inserted (acked, or localSeq <= the
// group's) and not removed (or removed by a local op newer than the group).  Members in
// document order (the reference sorts by ordinal); each one that yields an op joins a new
// group (same localSeq, kind, keys) at the tail of the queue.  io: [0] records written
// (-1: no pending group, -2: a capacity, -3: the document has failed), [1] text units,
// [2] props words.
__global__ void __launch_bounds__(MT_WAVE) k_regen(DevState st, int doc, mt_regen_rec *out, int cap, uint16_t *otext,
                                                   int tcap, uint32_t *oprops, int pcap, int32_t *io) {
    typedef TierLiveT<false> T;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
    const LdsLayout L = lds_layout(false, 0, st.B, 0, 0);
    DocT<T> d;
    load_doc(d, st, doc, (LDS_AS uint8_t *)smem_raw, L, 0, st.B, 0);
    if (d.status || d.g_n == 0) {
        if (lane() == 0) io[0] = d.status ? -3 : -1;
        return;
    }
    const int g = d.g_head;
    const int gw = lane() < MT_GRP_WORDS ? d.grp[g * MT_GRP_WORDS + lane()] : 0;   // the entry, lane j = word j
    const int ls = bcast(gw, 0), kind = bcast(gw, 1) & 0xFF;
    {   // sizing pass (reads only): output buffers too small leave the document untouched --
        // the caller retries with the sizes in io[1..3]
        int need_n = 0, need_t = 0, need_p = 0;
        for (int base = 0; base < d.n; base += MT_WAVE) {
            const int i = base + lane();
            const bool v = i < d.n;
            v4i a;
            u64 o;
            load_ao(d, i, v, a, o);
            const v4u b = d.Bv[v ? i : 0];
            const bool mem = v && pq_first(pq_get(d, v ? i : 0)) == g;
            const bool emit = mem && (kind != MT_OP_REMOVE || is_local_seq(a.z));
            const bool mk = (b.z & MT_MARKER_BIT) != 0;
            const int np = emit && kind == MT_OP_INSERT && b.y ? (int)prec(d, d.props_half, b.y)[0] : -1;
            need_n += __popcll(ballot(emit));
            need_t += wave_sum(emit && kind == MT_OP_INSERT && !mk ? a.x : 0);
            need_p += wave_sum(np >= 0 ? 1 + 2 * np : 0);
        }
        if (need_n > cap || need_t > tcap || need_p > pcap) {
            if (lane() == 0) {
                io[0] = -4;
                io[1] = need_n;
                io[2] = need_t;
                io[3] = need_p;
            }
            return;
        }
        if (d.g_n - 1 + need_n > d.LG) {   // the new groups need more ids: the live growth step first
            if (lane() == 0) {
                io[0] = -5;
                io[1] = d.g_n - 1 + need_n;
            }
            return;
        }
    }
    d.g_head = g % d.LG + 1;   // dequeue first: the new groups may reuse its table slot
    d.g_n--;
    int carry = 0, nout = 0, tu = 0, pw = 0;
    bool over = false;
    for (int base = 0; base < d.n && !over; base += MT_WAVE) {
        const int i = base + lane();
        const bool v = i < d.n;
        v4i a;
        u64 o;
        load_ao(d, i, v, a, o);
        const v4u b = d.Bv[v ? i : 0];
        const bool ins = !is_local_seq(a.y) || a.y - MT_LOCAL_BASE <= ls;
        const bool nrem = a.z == MT_RSEQ_NONE || (is_local_seq(a.z) && a.z - MT_LOCAL_BASE > ls);
        const int cl = v && ins && nrem ? a.x : 0;
        const int inc = wave_scan_incl(cl);
        const int pos = carry + inc - cl;
        const PendQ pq = pq_get(d, v ? i : 0);
        const bool mem = v && pq_first(pq) == g;
        for (u64 m = ballot(mem); m && !over; m &= m - 1) {
            const int j = first_lane(m);
            const int ij = base + j;
            PendQ oj = pq_pop(pq_bcast(pq, j));
            const int aj_x = bcast(a.x, j), aj_z = bcast(a.z, j);
            const bool emit = kind != MT_OP_REMOVE || is_local_seq(aj_z);
            if (emit) {
                const uint32_t bx = (uint32_t)bcast((int)b.x, j), by = (uint32_t)bcast((int)b.y, j);
                const bool mk = (bcast((int)b.z, j) & MT_MARKER_BIT) != 0;
                const int np = (kind == MT_OP_INSERT && by) ? (int)prec(d, d.props_half, by)[0] : -1;
                const int ng = (d.g_head - 1 + d.g_n) % d.LG + 1;
                const int tneed = kind == MT_OP_INSERT && !mk ? aj_x : 0;
                if (nout >= cap || d.g_n >= d.LG || !pq_push(oj, ng) || tu + tneed > tcap ||
                    pw + 1 + 2 * max(np, 0) > pcap) {
                    over = true;
                    break;
                }
                // same localSeq / kind / keys; joined now (its later splits append after it)
                if (lane() < MT_GRP_WORDS) d.grp[ng * MT_GRP_WORDS + lane()] = lane() == 10 ? d.next_uid : gw;
                d.g_n++;
                if (lane() == 0) {
                    mt_regen_rec r;
                    r.kind = kind;
                    r.pos1 = bcast(pos, j);
                    r.pos2 = kind == MT_OP_INSERT ? r.pos1 : r.pos1 + aj_x;
                    r.local_seq = ls;
                    r.text_off = mk ? bx : (uint32_t)tu;
                    r.text_len = (uint32_t)aj_x;
                    r.props_off = np >= 0 ? (uint32_t)pw : MT_NO_PROPS;
                    r.flags = mk ? MT_F_MARKER : 0u;
                    out[nout] = r;
                }
                if (kind == MT_OP_INSERT) {
                    gsync_rd();
                    if (!mk)
                        for (int q = lane(); q < aj_x; q += MT_WAVE) otext[tu + q] = text_base(d, d.text_half)[bx + q];
                    if (np >= 0) {
                        const GLB_AS uint32_t *pr = prec(d, d.props_half, by);
                        for (int q = lane(); q < 1 + 2 * np; q += MT_WAVE) oprops[pw + q] = pr[q];
                    }
                    tu += tneed;
                    pw += np >= 0 ? 1 + 2 * np : 0;
                }
                nout++;
            }
            if (lane() == 0) pq_put(d, ij, oj);
        }
        carry += bcast(inc, MT_WAVE - 1);
    }
    if (over) {   // the group table / a segment's FIFO is full (the buffers were sized above)
        d.status = MT_DOC_CAPACITY;
        d.cap_cause = 15;
    }
    store_doc(d, st, doc);
    if (lane() == 0) {
        io[0] = over ? -2 : nout;
        io[1] = tu;
        io[2] = pw;
    }
}

// Device time of a bulk read-out's kernels: up to two brackets of HIP events, created on first
// use; `timed` counts the brackets of the last read-out whose kernels have finished
// (read_timer: mt_last_text_ms, mt_last_props_ms, mt_last_locate, mt_last_dlog_ms, mt_last_tiles,
// mt_last_walk_ms).
struct ReadTimer {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int timed = 0;
    hipError_t begin(int k, hipStream_t s) {
        for (hipEvent_t *e : {&ev[2 * k], &ev[2 * k + 1]})
            if (!*e) {
                const hipError_t rc = hipEventCreate(e);
                if (rc != hipSuccess) return rc;
            }
        return hipEventRecord(ev[2 * k], s);
    }
    hipError_t end(int k, hipStream_t s) { return hipEventRecord(ev[2 * k + 1], s); }
    void destroy() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
};

struct mt_handle {
    int device = 0;
    bool live = false;       // live-client handle (mt_options.live_client)
    bool ordinals = false;   // segment ordinals kept (mt_options.segment_ordinals)
    uint32_t n_docs = 0;
    DevState st{};
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_load = nullptr, ev_load1 = nullptr;
    bool load_timed = false;   // ev_load / ev_load1 bracket the last snapshot load's kernels
    // mt_get_texts, mt_get_prop_runs_bulk: around the counting pass, around the gather; the bulk
    // segment read-outs: around their kernel
    ReadTimer tm_txt, tm_prp, tm_loc, tm_dlg, tm_tile, tm_walk;
    uint32_t *d_rst = nullptr;   // mt_delta_log_reset_docs: the listed documents (rst_cap of them)
    uint32_t rst_cap = 0;
    int64_t loc_n = 0, loc_host = 0;   // queries of the last segment read-out, of them answered by the host path
    int64_t wv_n = 0, wv_host = 0, wv_skip = 0;   // queries of the last walk in a view, of them answered by the
                                                  // host path / started by the table-based page seek
    int64_t tile_n = 0, tile_rows = 0;   // queries of the last marker query, rows its kernel examined
    // documents per workgroup of the LDS-tier replay (env MT_WPG=2 for two): measured on C2
    // the CU saturates at 16 resident documents (16 -> 18 per CU: 61.8 -> 64.6 ms)
    int wpg = 1;
    float last_ms = 0.f;
    bool timed = false;      // ev0/ev1 bracket a launch not yet read by mt_sync
    std::string err;
    mt_checksum *d_sums = nullptr;
    int64_t *d_seed_off = nullptr;   // initial contents kept on device for mt_reset
    uint16_t *d_seed = nullptr;
    TierCaps lds{0, 0, 0, 0};        // LDS-tier capacities (S == 0: tier disabled)
    PagedCaps pg_tight{0, 0, 0, 1, 1, 0};   // tight paged tier (PP == 0: off)
    PagedCaps pg_full{0, 0, 0, 0, 1, 0};    // paged tier at the HBM capacities
    int paged_slices = 0;                   // mt_options.paged_slices
    int pg_resident = 0;                    // documents resident at once in a tight paged launch
    // growth step (mt_settle): the batch whose launches may have handed documents to it, the
    // big region's capacities (PP == 0: none yet) and its slots, the documents moved there
    struct mt_batch *pending = nullptr;
    PagedCaps big_caps{0, 0, 0, 0, 3, 0, 1};
    std::vector<int32_t> bslot_h;           // host mirror of st.bslot
    uint32_t n_big = 0;                     // documents with a slot in the big region
    int max_cli = 0;                        // largest |short client id| any batch / load / generation used
                                            // (<= 127: the tight tier may pack its table, PagedCaps.packed)
    uint32_t grown_last = 0, grow_rounds_last = 0;
};
struct mt_batch {
    mt_handle *owner = nullptr;   // the handle whose growth step still needs this batch
    int device = 0;
    uint32_t n_docs = 0;
    uint64_t n_ops = 0, text_len = 0, props_len = 0;
    int64_t *off = nullptr;
    mt_op_rec *ops = nullptr;
    uint16_t *text = nullptr;
    uint32_t *props = nullptr;
    int32_t *order = nullptr;     // dispatch order (DevState.order), null when lengths are equal
};
// The batch's device arrays at the sizes it holds (mt_batch_free releases them).
static hipError_t batch_alloc(mt_batch *b) {
    hipError_t e = hipMalloc(&b->off, ((size_t)b->n_docs + 1) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc(&b->ops, std::max<uint64_t>(b->n_ops, 1) * sizeof(mt_op_rec));
    if (e == hipSuccess) e = hipMalloc(&b->text, std::max<uint64_t>(b->text_len, 1) * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&b->props, std::max<uint64_t>(b->props_len, 1) * sizeof(uint32_t));
    return e;
}
// Longest-first dispatch order of a batch whose documents differ in length (stable: equal
// lengths keep index order); none when every document has the same number of messages.
static bool set_order(mt_batch *b, const int64_t *off) {
    const uint32_t n = b->n_docs;
    bool equal = true;
    for (uint32_t d = 1; d < n && equal; d++) equal = off[d + 1] - off[d] == off[1] - off[0];
    if (equal) return true;
    std::vector<int32_t> ord(n);
    for (uint32_t d = 0; d < n; d++) ord[d] = (int32_t)d;
    std::stable_sort(ord.begin(), ord.end(),
                     [&](int32_t x, int32_t y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });
    return hipMalloc(&b->order, (size_t)n * 4) == hipSuccess &&
           hipMemcpy(b->order, ord.data(), (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess;
}

#define HIPCHK(h, x)                                                               \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            if (h) (h)->err = std::string(#x) + ": " + hipGetErrorString(e_);      \
            return MT_E_HIP;                                                       \
        }                                                                          \
    } while (0)

// Device memory that a function allocates and frees itself (n elements of T; bytes by
// default): freed on every return, HIPCHK's included.  release() hands it to another owner.
template <class T = uint8_t> struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T)); }
    T *release() {
        T *q = p;
        p = nullptr;
        return q;
    }
};

// ---------------------------------------------------------------- kernel variants
// One row per entry of MT_VARIANTS: the kernel and the facts that select it and size its
// dynamic LDS, read off the tier type that instantiates it -- a row cannot disagree with its
// kernel.  Every launch of a replay / generate / load-convert kernel asks pick_flat or
// pick_paged for its row and its LDS bytes and goes through launch_variant.
enum KFamily { K_REPLAY, K_REPLAY_PAGED, K_GENERATE, K_GENERATE_PAGED, K_LOAD_CONVERT };
#define MT_FAM_k_replay K_REPLAY
#define MT_FAM_k_replay_paged K_REPLAY_PAGED
#define MT_FAM_k_generate K_GENERATE
#define MT_FAM_k_generate_paged K_GENERATE_PAGED
#define MT_FAM_k_load_convert K_LOAD_CONVERT
struct Variant {
    const char *name;
    const void *(*kernel)();
    KFamily fam;
    bool log;                 // T::kLog
    bool lds, live;           // flat tiers: T::kLds, T::kLive
    int wpg;                  // k_replay: documents per workgroup
    int ob;                   // paged tiers: sizeof(T::O_v), 4 for a narrow tier
    bool big, packed, hm;     // T::kBig, T::kPacked, T::kHM
    int PP, PH, UT;           // T::kPP / kPH / kUT (0: the launch's)
};
template <class T, int WPG = 1>
static constexpr Variant variant_row(const char *name, const void *(*kernel)(), KFamily fam) {
    if constexpr (T::kPaged)
        return Variant{name, kernel, fam, T::kLog, true, false, 1, (int)sizeof(typename T::O_v),
                       T::kBig, T::kPacked, T::kHM, T::kPP, T::kPH, T::kUT};
    else
        return Variant{name, kernel, fam, T::kLog, T::kLds, T::kLive, WPG, 0, false, false, false, 0, 0, 0};
}
#define MT_VARIANT_ROW(n, k, targs) variant_row<MT_UNPAREN targs>(#n, mtk_##n, MT_FAM_##k),
static const Variant kVariants[] = {MT_VARIANTS(MT_VARIANT_ROW)};

struct HandleFacts {
    bool log, ordinals, live;   // st.DL > 0, mt_options.segment_ordinals, mt_options.live_client
    int wpg;                    // documents per workgroup asked of the LDS-tier replay
};
static HandleFacts facts(const mt_handle *h) { return HandleFacts{h->st.DL > 0, h->ordinals, h->live, h->wpg}; }
struct Pick {
    const Variant *v;   // nullptr: the library has no such kernel (an error, never a fall-back)
    size_t lds;         // its dynamic LDS bytes
};

// The flat family (k_replay, k_generate).  caps.S > 0: the LDS tier's launch, else the HBM
// tier's.  The generator keeps neither a delta log nor live state; two documents per
// workgroup exist for the plain observer replay only (any other handle runs one).
// LDS: WPG slices of the kernel's own lds_layout(T::kLds, S, B, H, gen_words).
static Pick pick_flat(KFamily fam, const HandleFacts &f, const TierCaps &c, int gen_words) {
    const bool lds = c.S > 0, gen = fam == K_GENERATE;
    const bool live = !gen && f.live, log = !gen && f.log;
    const Variant *v = nullptr;
    for (const int wpg : {lds && !gen ? f.wpg : 1, 1})
        for (const Variant &r : kVariants)
            if (!v && r.fam == fam && r.lds == lds && r.live == live && r.log == log && r.wpg == wpg) v = &r;
    return Pick{v, v ? v->wpg * (size_t)lds_layout(v->lds, c.S, c.B, c.H, gen_words).total : 0};
}

// Documents of many pages replay with their page metadata in HBM (TierPagedT kHM: no LDS per
// page instead of 12 bytes, so more of them share a CU); the bench's C3 / C4 documents (< 300
// pages) keep it in LDS (no global load on their page searches).  Delta-logging handles take
// the kHM tier too (P_HM_LOG, P_BIG_HM_LOG); segment-ordinal handles keep the LDS metadata.
#ifndef MT_HM_PAGES
#define MT_HM_PAGES 512
#endif
// The kernel's own paged_layout call: k_replay_paged substitutes its compile-time capacities
// (eff_caps) and passes kPacked / kHM; k_generate_paged adds the generator's words;
// k_load_convert neither.
static size_t paged_lds_bytes(const Variant &v, PagedCaps pc, int gen_words) {
    if (v.fam != K_REPLAY_PAGED) return paged_layout(pc.PP, pc.PH, pc.UT, gen_words, v.ob).total;
    if (v.PP > 0) pc.PP = v.PP;
    if (v.PH > 0) pc.PH = v.PH;
    if (v.UT > 0) pc.UT = v.UT;
    return paged_layout(pc.PP, pc.PH, pc.UT, 0, v.ob, v.packed, v.hm).total;
}
// The paged family (k_replay_paged, k_generate_paged, k_load_convert); big: the launch serves
// the big region's documents (the growth step's).  A kernel whose compile-time capacities are
// the launch's wins over the run-time one (the bench's C3 and C4 tight tiers, DESIGN section
// 11).  The generator keeps no delta log; load-convert compiles it in for the canonical
// ordinals only.  sizing: mt_create's occupancy query, which sizes the sliced schedule by the
// tier's plain run-time kernel whatever the launches later run.
static Pick pick_paged(KFamily fam, const HandleFacts &f, const PagedCaps &pc, bool big, int gen_words,
                       bool sizing = false) {
    const bool log = fam == K_REPLAY_PAGED ? f.log : (fam == K_LOAD_CONVERT ? f.ordinals : false);
    const bool hm = fam == K_REPLAY_PAGED && !sizing && !pc.packed && !pc.narrow && !f.ordinals &&
                    pc.PP >= MT_HM_PAGES;
    const Variant *v = nullptr;
    for (const bool fixed : {true, false})
        for (const Variant &r : kVariants) {
            if (v || r.fam != fam || r.log != log || (r.ob == 4) != (pc.narrow != 0) || r.big != big ||
                r.packed != (pc.packed != 0) || r.hm != hm || (r.PP > 0) != fixed)
                continue;
            if (!fixed || (!sizing && r.PP == pc.PP && r.PH == pc.PH && r.UT == pc.UT)) v = &r;
        }
    return Pick{v, v ? paged_lds_bytes(*v, pc, gen_words) : 0};
}

// A launch that needs more than the 64 KiB every kernel may use raises the kernel's
// MaxDynamicSharedMemorySize first.  The attribute belongs to the process (per device), not to
// a handle: the largest value set so far is kept per kernel and never lowered, so a handle with
// a smaller layout cannot take the limit away from under another one.
static hipError_t raise_lds_limit(const void *kernel, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> set;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = set[{dev, kernel}];
    if (lds <= cur) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}
// One wave per document, p.v->wpg documents per workgroup; args: the kernel's exact parameters
// (errors are read with hipGetLastError as for hipLaunchKernelGGL).
static hipError_t launch_variant(const Pick &p, uint32_t n_docs, hipStream_t s, void **args) {
    if (!p.v) return hipErrorInvalidDeviceFunction;
    const void *k = p.v->kernel();
    const hipError_t e = raise_lds_limit(k, p.lds);
    if (e != hipSuccess) return e;
    const uint32_t w = (uint32_t)p.v->wpg;
    (void)hipLaunchKernel(k, dim3((n_docs + w - 1) / w), dim3(MT_WAVE * w), args, p.lds, s);
    return hipGetLastError();
}
static hipError_t launch_replay(const Pick &p, mt_handle *h, const mt_batch *b, TierCaps caps) {
    void *a[] = {&h->st, (void *)&b->ops, (void *)&b->off, (void *)&b->text, (void *)&b->props, &caps};
    return launch_variant(p, h->n_docs, h->stream, a);
}

static int mt_settle(mt_handle *h);
// waits for the stream and finishes a pending growth step (API entry points that read state or
// enqueue work: a growth step's launches must come before anything else)
#define SETTLE(h)                          \
    do {                                   \
        const int rc_ = mt_settle(h);      \
        if (rc_) return rc_;               \
    } while (0)

static TierCaps glb_caps(const mt_handle *h) { return TierCaps{0, h->st.B, 0, h->lds.S > 0 ? 1 : 0}; }
// the live handle's HBM tier: documents that could outgrow it go to the live growth step
static TierCaps live_caps(const mt_handle *h) {
    TierCaps c = glb_caps(h);
    c.grow = 1;
    return c;
}

// A props record [count | combine << 16, (key, value) x count] lies inside the arena.
static bool props_rec_ok(const uint32_t *props, uint64_t props_len, uint32_t off) {
    if (off == MT_NO_PROPS) return true;
    if ((uint64_t)off >= props_len) return false;
    const uint64_t cnt = props[off] & 0xFFFFu;
    uint64_t end = (uint64_t)off + 1 + 2 * cnt;
    if ((props[off] >> 16) == MT_COMBINE_TABLE) {   // + [n, absent, (old, new) x n]
        if (end + 2 > props_len) return false;
        end += 2 + 2 * (uint64_t)props[end];
    }
    return end <= props_len;
}
// Host-side bounds check of a batch (MT_E_INVALID instead of a device fault): per-document
// offsets monotonic inside [0, n_ops], every insert payload inside the text arena, every
// props record inside the props arena, known op kinds.
// (one pass over the records: also the largest |short client id| they name, for max_cli)
static std::string validate_batch(uint32_t n_docs, const int64_t *off, const mt_op_rec *ops, uint64_t n_ops,
                                  uint64_t text_len, const uint32_t *props, uint64_t props_len, bool live,
                                  int &max_cli) {
    if (off[0] < 0) return "doc_op_off[0] < 0";
    for (uint32_t d = 0; d < n_docs; d++)
        if (off[d + 1] < off[d]) return "doc_op_off not monotonic at document " + std::to_string(d);
    if ((uint64_t)off[n_docs] > n_ops) return "doc_op_off exceeds n_ops";
    int mc = max_cli;
    for (uint64_t k = (uint64_t)off[0]; k < (uint64_t)off[n_docs]; k++) {
        const mt_op_rec &o = ops[k];
        mc = std::max(mc, std::abs((int)(int16_t)o.client));
        if (o.kind > MT_OP_LOAD_ALIASED) return "op " + std::to_string(k) + ": unknown kind";
        if (o.kind >= MT_OP_LOAD_REMOVED && !(o.flags & MT_F_LOAD))
            return "op " + std::to_string(k) + ": summary-load record without MT_F_LOAD";
        if ((o.flags & (MT_F_LOCAL | MT_F_ACK)) && !live)
            return "op " + std::to_string(k) + ": local / ack record on a handle without live_client";
        if ((o.flags & MT_F_LOCAL) && (o.flags & MT_F_ACK))
            return "op " + std::to_string(k) + ": both MT_F_LOCAL and MT_F_ACK";
        if ((o.flags & MT_F_LOCAL) && o.client != 0)
            return "op " + std::to_string(k) + ": a local op's client must be the local client (short id 0)";
        if (o.kind == MT_OP_INSERT && !(o.flags & MT_F_MARKER)) {
            if (o.pos2 < 0 || (uint64_t)o.payload + (uint64_t)o.pos2 > text_len)
                return "op " + std::to_string(k) + ": insert payload outside the text arena";
        }
        if ((o.kind == MT_OP_INSERT || o.kind == MT_OP_ANNOTATE) && !props_rec_ok(props, props_len, o.props))
            return "op " + std::to_string(k) + ": props record outside the props arena";
    }
    max_cli = mc;
    return std::string();
}

// ---------------------------------------------------------------- bulk read-out harness
// What mt_get_texts, mt_get_prop_runs_bulk and the bulk segment read-outs (locate) share; each
// keeps its kernels, its error text and, for locate, its host path.

// The queries of a bulk read-out: fewer than 2^31, each naming a document of the handle
// (docs == nullptr: query q reads document q).
static int check_queries(mt_handle *h, const char *name, uint32_t n, const uint32_t *docs) {
    if (n > 0x7FFFFFFFu || (!docs && n > h->n_docs)) return MT_E_INVALID;
    for (uint32_t q = 0; docs && q < n; q++)
        if (docs[q] >= h->n_docs) {
            h->err = std::string(name) + ": query " + std::to_string(q) + ": no document " + std::to_string(docs[q]);
            return MT_E_INVALID;
        }
    return 0;
}
// The query columns on the device, one allocation: `extra` bytes of the read-out's own (a
// multiple of 8, 16-byte aligned), then up to four columns of n words; an absent column's
// pointer is null, as the kernels expect.
struct QueryCols {
    DevBuf<> buf;
    uint8_t *extra = nullptr;
    void *col[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t upload(uint32_t n, std::initializer_list<const void *> cols, size_t extra_bytes) {
        hipError_t e = buf.alloc(extra_bytes + cols.size() * (size_t)n * 4);
        extra = buf.p;
        int i = 0;
        for (const void *c : cols) {
            void *d = buf.p + extra_bytes + (size_t)i * n * 4;
            if (c && e == hipSuccess) e = hipMemcpy(d, c, (size_t)n * 4, hipMemcpyHostToDevice);
            col[i++] = c ? d : nullptr;
        }
        return e;
    }
};
static int read_timer(mt_handle *h, const ReadTimer &t, float *out /* [2] */) {
    out[0] = out[1] = 0.f;
    if (t.timed >= 1) HIPCHK(h, hipEventElapsedTime(&out[0], t.ev[0], t.ev[1]));
    if (t.timed >= 2) HIPCHK(h, hipEventElapsedTime(&out[1], t.ev[2], t.ev[3]));
    return 0;
}
// No query: every offset array is its single 0.
static int empty_offsets(mt_handle *h, std::initializer_list<int64_t *> off, bool device) {
    for (int64_t *o : off)
        if (device)
            HIPCHK(h, hipMemset(o, 0, 8));
        else
            o[0] = 0;
    return 0;
}
// k streams of per-query counts (device, n each) -> their exclusive prefix sums off[i][n + 1]
// and totals: on the host for host results (as mt_extract_snapshots takes them), by k_text_scan
// for device results (off[i]: device arrays).  Returns with the stream idle.
static int scan_counts(mt_handle *h, uint32_t n, int k, int64_t *const *d_cnt, int64_t *const *off, bool device,
                       int64_t *total) {
    if (device) {
        for (int i = 0; i < k; i++) {
            hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(1024), 0, h->stream, d_cnt[i], (int)n, off[i]);
            HIPCHK(h, hipGetLastError());
        }
        for (int i = 0; i < k; i++)
            HIPCHK(h, hipMemcpyAsync(&total[i], off[i] + n, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return 0;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < k; i++) {
        HIPCHK(h, hipMemcpy(off[i] + 1, d_cnt[i], (size_t)n * 8, hipMemcpyDeviceToHost));
        off[i][0] = 0;
        for (uint32_t q = 0; q < n; q++) off[i][q + 1] += off[i][q];
        total[i] = off[i][n];
    }
    return 0;
}
// With the totals known: RO_DONE without an output to fill (sizing only) or without results,
// MT_E_OVERFLOW (message from overflow_msg) when the outputs are too small -- they stay
// untouched, the offsets are already written -- else RO_GATHER.
enum { RO_DONE = 0, RO_GATHER = 1 };
template <class Msg> static int after_counts(mt_handle *h, bool sizing, bool fits, bool empty, Msg overflow_msg) {
    if (sizing) return RO_DONE;
    if (!fits) {
        h->err = overflow_msg();
        return MT_E_OVERFLOW;
    }
    return empty ? RO_DONE : RO_GATHER;
}
// Where a gather writes: the caller's device array, or (host results) device memory of this
// call that copy_out then copies to the caller's host array.
template <class T> struct OutStage {
    DevBuf<T> own;
    T *p = nullptr;
    hipError_t open(void *caller_dev, bool device, size_t count) {
        const hipError_t e = device ? hipSuccess : own.alloc(count);
        p = device ? (T *)caller_dev : own.p;
        return e;
    }
    hipError_t copy_out(void *host, size_t count) const {
        return own.p && count ? hipMemcpy(host, own.p, count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    }
};

extern "C" {

mt_handle *mt_create(uint32_t n_docs, const mt_options *opt) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return nullptr;
    mt_options o{};
    if (opt) o = *opt;
    // the default handle is unbounded: the paged layout with the growth step behind it, at
    // small starting capacities (a flat-only handle is opt-in: page_capacity < 0); live
    // handles stay flat
    const bool dflt_paged = o.page_capacity == 0 && o.live_client == 0;
    if (dflt_paged) {
        o.page_capacity = 64;
        if (o.page_heap_capacity <= 0) o.page_heap_capacity = 256;
        if (o.unsettled_capacity <= 0) o.unsettled_capacity = 256;
        if (o.uid_capacity <= 0) o.uid_capacity = 8192;
        if (o.seg_capacity <= 0) o.seg_capacity = 512;
    }
    if (o.page_capacity < 0) o.page_capacity = 0;
    auto *h = new mt_handle();
    h->device = o.device;
    h->n_docs = n_docs;
    if (hipSetDevice(h->device) != hipSuccess) {
        delete h;
        return nullptr;
    }
    DevState &st = h->st;
    st.n_docs = (int32_t)n_docs;
    st.S = o.seg_capacity > 0 ? o.seg_capacity : 2048;
    st.B = o.block_capacity > 0 ? o.block_capacity : std::max(64, st.S / 2);
    st.B = (st.B + 63) / 64 * 64;
    st.H = o.heap_capacity > 0 ? o.heap_capacity : 2 * st.S;
    st.T = o.text_capacity > 0 ? o.text_capacity : 32768;
    st.P = o.props_capacity > 0 ? o.props_capacity : st.S + 2 * MT_WAVE;
    st.DL = o.delta_log_capacity > 0 ? o.delta_log_capacity : 0;
    st.DLR = st.DL > 0 && o.delta_log_mode == 1 ? 1 : 0;
    h->ordinals = o.segment_ordinals != 0;
    if (h->ordinals && !st.DLR) {   // ordinals ride on the rich log
        delete h;
        return nullptr;
    }
    if (const char *e = getenv("MT_WPG")) h->wpg = atoi(e) == 1 ? 1 : 2;
    h->live = o.live_client != 0;
    if (h->live && o.page_capacity > 0) {   // live documents replay from the flat HBM tier
        delete h;
        return nullptr;
    }
    // live handles stage in LDS (TierLiveLdsT, then TierLiveT) only when asked for explicitly
    if (o.lds_seg_capacity > 0 || (o.lds_seg_capacity == 0 && !h->live)) {
        int S_l = o.lds_seg_capacity > 0 ? o.lds_seg_capacity : 192;
        S_l = std::min(S_l, st.S);
        h->lds.S = S_l;
        h->lds.B = std::min(st.B, std::max(64, (S_l / 2 + 32 + 15) / 16 * 16));
        // zamboni heap in LDS: entries older than minSeq are popped as ops arrive, so the
        // heap stays far below S_l (C2 needs < 96 at S_l 192: 0 hand-overs); a smaller heap
        // is a smaller LDS footprint = more documents per CU (profiles/r1 sweep: 74.9 -> 68.9 ms)
        h->lds.H = std::min(st.H, std::max(64, S_l / 2));
        if (lds_layout(true, h->lds.S, h->lds.B, h->lds.H, 0).total > 60 * 1024) h->lds = TierCaps{0, 0, 0, 0};
    }
    if (o.page_capacity > 0) {
        st.PP = std::min(o.page_capacity, 65535);
        st.PH = o.page_heap_capacity > 0 ? o.page_heap_capacity : 1024;
        st.UT = o.unsettled_capacity > 0 ? o.unsettled_capacity : 256;
        st.UM = std::min(o.uid_capacity > 0 ? o.uid_capacity : 65536, 1 << 24);
        st.UM = std::max(st.UM, 256);
        h->pg_full = PagedCaps{st.PP, st.PH, st.UT, 0, 1, 0, 1};
        const PagedCaps t{o.lds_page_capacity > 0 ? std::min(o.lds_page_capacity, st.PP) : st.PP,
                          o.lds_page_heap_capacity > 0 ? std::min(o.lds_page_heap_capacity, st.PH) : st.PH,
                          o.lds_unsettled_capacity > 0 ? std::min(o.lds_unsettled_capacity, st.UT) : st.UT, 1, 1,
                          o.lds_narrow_overlap ? 1 : 0};
        if (t.PP < st.PP || t.PH < st.PH || t.UT < st.UT || t.narrow) {
            h->pg_tight = t;
            h->pg_full.stage = 2;
        }
        // one document's paged state staged in LDS: up to the CU's 160 KiB (fewer
        // documents per CU above 64 KiB)
        const size_t lb = paged_layout(st.PP, st.PH, st.UT, 2 * 65, 8).total;
        if (lb > 160 * 1024) {
            delete h;
            return nullptr;
        }
        // a device whose kernels cannot have that much fails the creation, not the first launch
        // (asked of the last tier's kernel; every launch raises its own kernel's limit itself)
        if (raise_lds_limit(pick_paged(K_REPLAY_PAGED, facts(h), h->pg_full, false, 0, true).v->kernel(), lb) !=
            hipSuccess) {
            delete h;
            return nullptr;
        }
        // documents resident at once in the first paged launch (the sliced schedule's round)
        h->paged_slices = std::min(std::max(o.paged_slices, 0), 256);
        if (h->paged_slices > 1) {
            const PagedCaps &c = h->pg_tight.PP ? h->pg_tight : h->pg_full;
            const Pick p = pick_paged(K_REPLAY_PAGED, facts(h), c, false, 0, true);
            int per_cu = 0, cus = 0;
            hipDeviceProp_t prop;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p.v->kernel(), MT_WAVE, p.lds) == hipSuccess &&
                hipGetDeviceProperties(&prop, h->device) == hipSuccess)
                cus = prop.multiProcessorCount;
            h->pg_resident = per_cu * cus;
        }
    }
    const size_t N = n_docs;
    bool ok = true;
    auto alloc = [&](void **p, size_t bytes) {
        if (!ok) return;
        if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) ok = false;
    };
    alloc((void **)&st.hdr, N * sizeof(DocHdr));
    alloc((void **)&st.segA, N * st.S * sizeof(int4));
    alloc((void **)&st.segO, N * st.S * sizeof(u64));
    alloc((void **)&st.segB, N * st.S * sizeof(uint4));
    alloc((void **)&st.cnt, N * MT_LV * st.B);
    alloc((void **)&st.flg, N * st.B);
    alloc((void **)&st.heap, N * (size_t)(st.H + 1) * sizeof(int2));
    alloc((void **)&st.oslot, N * (size_t)(2 * MT_OSLOTS) * sizeof(int32_t));
    alloc((void **)&st.text, N * 2 * (size_t)st.T * sizeof(uint16_t));
    alloc((void **)&st.props, N * 2 * (size_t)st.P * MT_PREC * sizeof(uint32_t));
    if (st.DL) alloc((void **)&st.dlog, N * (size_t)st.DL * sizeof(int32_t));
    alloc((void **)&h->d_sums, N * sizeof(mt_checksum));
    alloc((void **)&st.retry, N * sizeof(int32_t));
    alloc((void **)&st.resume, N * sizeof(int64_t));
    alloc((void **)&st.stats, MT_STATS_WORDS * sizeof(uint32_t));
#ifdef MT_PROF
    alloc((void **)&st.prof, 128 * sizeof(unsigned long long));
    if (ok) ok = hipMemset(st.prof, 0, 128 * sizeof(unsigned long long)) == hipSuccess;
#endif
    if (h->ordinals) {
        alloc((void **)&st.ordS, N * (size_t)st.S * sizeof(uint16_t));
        alloc((void **)&st.ordB, N * (size_t)MT_LV * st.B * sizeof(uint16_t));
    }
    if (h->live) {
        alloc((void **)&st.live, N * 4 * sizeof(int32_t));
        st.LG = std::min(std::max(o.live_group_capacity > 0 ? o.live_group_capacity : 1024, 16), 65535);
        alloc((void **)&st.grp, N * (size_t)(st.LG + 1) * MT_GRP_WORDS * sizeof(int32_t));
        alloc((void **)&st.segP, N * (size_t)st.S * sizeof(PendQ));
    }
    if (st.PP > 0) {
        const size_t slots = N * (size_t)st.PP * MT_PG_SLOTS;
        alloc((void **)&st.pgA, slots * sizeof(int4));
        alloc((void **)&st.pgO, slots * sizeof(u64));
        alloc((void **)&st.pgB, slots * sizeof(uint4));
        alloc((void **)&st.pgMeta, N * st.PP * sizeof(PageMeta));
        alloc((void **)&st.pgDir, N * st.PP * sizeof(uint16_t));
        alloc((void **)&st.pgCnt, N * MT_LV * (size_t)st.PP);
        alloc((void **)&st.pgHeap, N * (size_t)(st.PH + 1) * sizeof(int2));
        alloc((void **)&st.pgUtPage, N * (size_t)st.UT * sizeof(int32_t));
        alloc((void **)&st.pgUtA, N * (size_t)st.UT * sizeof(int4));
        alloc((void **)&st.pgUtO, N * (size_t)st.UT * sizeof(u64));
        alloc((void **)&st.pgUmap, N * (size_t)st.UM * sizeof(uint16_t));
        st.OA = o.overlap_arena_capacity > 0 ? std::min(std::max(o.overlap_arena_capacity, 64), 1 << 30) & ~7
                                              : MT_OVF_ARENA;
        alloc((void **)&st.pgOvf, N * (size_t)st.OA * sizeof(uint16_t));
        if (st.pgOvf) hipMemset(st.pgOvf, 0, N * (size_t)st.OA * sizeof(uint16_t));
        if (h->ordinals) {
            alloc((void **)&st.pgOS, slots * sizeof(uint16_t));
            alloc((void **)&st.pgOL, N * (size_t)st.PP * MT_PG_OLB * sizeof(uint16_t));
            alloc((void **)&st.pgOU, N * (size_t)MT_LV * st.PP * sizeof(uint16_t));
        }
    }
    if (!ok || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipEventCreate(&h->ev_load) != hipSuccess || hipEventCreate(&h->ev_load1) != hipSuccess) {
        mt_destroy(h);
        return nullptr;
    }
    if (mt_load_initial_text(h, nullptr, nullptr) != 0) {
        mt_destroy(h);
        return nullptr;
    }
    return h;
}

static void free_region(PagedRegion &R) {
    void *ps[] = {R.A, R.O, R.B, R.meta, R.dir, R.cnt, R.heap, R.upage, R.uA, R.uO, R.oS, R.oL, R.oU, R.text, R.props, R.umap, R.ovf};
    for (void *p : ps)
        if (p) hipFree(p);
    R = PagedRegion{};
}

void mt_destroy(mt_handle *h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->pending) h->pending->owner = nullptr;
    free_region(h->st.big);
    if (h->st.bslot) hipFree(h->st.bslot);
    DevState &st = h->st;
    void *ps[] = {st.hdr, st.segA, st.segO, st.segB, st.cnt, st.flg, st.heap, st.text, st.props, st.dlog, h->d_sums,
                  h->d_seed_off, h->d_seed, st.retry, st.stats, st.resume, st.pgA, st.pgO, st.pgB, st.pgMeta,
                  st.pgDir, st.pgCnt, st.pgHeap, st.pgUtPage, st.pgUtA, st.pgUtO, st.pgUmap, st.pgOvf, st.oslot,
                  st.live, st.grp, st.segP, st.ordS, st.ordB, st.pgOS, st.pgOL, st.pgOU, st.prof};
    for (void *p : ps)
        if (p) hipFree(p);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->ev_load) hipEventDestroy(h->ev_load);
    if (h->ev_load1) hipEventDestroy(h->ev_load1);
    for (ReadTimer *t : {&h->tm_txt, &h->tm_prp, &h->tm_loc, &h->tm_dlg, &h->tm_tile, &h->tm_walk}) t->destroy();
    if (h->d_rst) hipFree(h->d_rst);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

const char *mt_last_error(const mt_handle *h) { return h ? h->err.c_str() : "null handle"; }
uint32_t mt_num_docs(const mt_handle *h) { return h ? h->n_docs : 0; }

// startCollaboration's window for the listed documents (mt_start_collaboration)
__global__ void k_set_window(DevState st, const int32_t *ms, const int32_t *cs) {
    const uint32_t doc = blockIdx.x * blockDim.x + threadIdx.x;
    if (doc >= (uint32_t)st.n_docs || ms[doc] < 0) return;
    st.hdr[doc].min_seq = ms[doc];
    st.hdr[doc].cur_seq = cs[doc];
    st.hdr[doc].heap_n = 0;
}

int mt_start_collaboration(mt_handle *h, const int32_t *min_seq, const int32_t *cur_seq) {
    if (!h || !min_seq || !cur_seq) return MT_E_INVALID;
    for (uint32_t d = 0; d < h->n_docs; d++)
        if (min_seq[d] >= 0 && cur_seq[d] < min_seq[d]) {
            h->err = "mt_start_collaboration: document " + std::to_string(d) + " has currentSeq < minSeq";
            return MT_E_INVALID;
        }
    SETTLE(h);
    DevBuf<int32_t> d_w;   // [min_seq | cur_seq]
    HIPCHK(h, d_w.alloc((size_t)h->n_docs * 2 + 2));
    HIPCHK(h, hipMemcpyAsync(d_w.p, min_seq, (size_t)h->n_docs * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_w.p + h->n_docs, cur_seq, (size_t)h->n_docs * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_set_window, dim3((h->n_docs + 255) / 256), dim3(256), 0, h->stream, h->st, d_w.p,
                       d_w.p + h->n_docs);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int mt_load_initial_text(mt_handle *h, const int64_t *seed_off, const uint16_t *seed_text) {
    if (!h) return MT_E_INVALID;
    SETTLE(h);
    if (h->d_seed_off) hipFree(h->d_seed_off);
    if (h->d_seed) hipFree(h->d_seed);
    h->d_seed_off = nullptr;
    h->d_seed = nullptr;
    if (seed_off) {
        if (seed_off[0] != 0) {
            h->err = "mt_load_initial_text: seed_off[0] != 0";
            return MT_E_INVALID;
        }
        for (uint32_t d = 0; d < h->n_docs; d++)
            if (seed_off[d + 1] < seed_off[d]) {
                h->err = "mt_load_initial_text: seed_off not monotonic";
                return MT_E_INVALID;
            }
        if (seed_off[h->n_docs] > 0 && !seed_text) {
            h->err = "mt_load_initial_text: null seed_text";
            return MT_E_INVALID;
        }
        const size_t n = seed_off[h->n_docs];
        HIPCHK(h, hipMalloc(&h->d_seed_off, (h->n_docs + 1) * sizeof(int64_t)));
        HIPCHK(h, hipMalloc(&h->d_seed, std::max<size_t>(n, 1) * sizeof(uint16_t)));
        HIPCHK(h, hipMemcpy(h->d_seed_off, seed_off, (h->n_docs + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        if (n) HIPCHK(h, hipMemcpy(h->d_seed, seed_text, n * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    int rc = mt_reset(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int mt_reset(mt_handle *h) {
    if (!h) return MT_E_INVALID;
    if (h->pending) SETTLE(h);
    HIPCHK(h, hipSetDevice(h->device));
    if (h->n_big > 0) {   // every document starts over in the main arrays (k_init clears bslot)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        free_region(h->st.big);
        h->big_caps = PagedCaps{0, 0, 0, 0, 3, 0, 1};
        h->bslot_h.assign(h->n_docs, -1);
        h->n_big = 0;
    }
    if (h->st.DL) HIPCHK(h, hipMemsetAsync(h->st.dlog, 0, (size_t)h->n_docs * h->st.DL * 4, h->stream));
    hipLaunchKernelGGL(k_init, dim3(h->n_docs), dim3(MT_WAVE), 0, h->stream, h->st, h->d_seed_off, h->d_seed);
    HIPCHK(h, hipGetLastError());
    return 0;
}

mt_batch *mt_batch_upload(mt_handle *h, const int64_t *doc_op_off, const mt_op_rec *ops,
                          uint64_t n_ops, const uint16_t *text, uint64_t text_len,
                          const uint32_t *props, uint64_t props_len) {
    if (!h || !doc_op_off || (n_ops && !ops) || (text_len && !text) || (props_len && !props)) {
        if (h) h->err = "mt_batch_upload: null array";
        return nullptr;
    }
    // the kernels index ops, text and props straight from these values: reject anything
    // that would read outside the arrays (remote ops are trusted for their semantics, not
    // for memory safety)
    int max_cli = h->max_cli;
    std::string bad = validate_batch(h->n_docs, doc_op_off, ops, n_ops, text_len, props, props_len, h->live, max_cli);
    if (!bad.empty()) {
        h->err = "mt_batch_upload: " + bad;
        return nullptr;
    }
    h->max_cli = max_cli;   // (over the records the documents replay)
    if (hipSetDevice(h->device) != hipSuccess) return nullptr;
    auto *b = new mt_batch();
    b->device = h->device;
    b->n_docs = h->n_docs;
    b->n_ops = n_ops;
    b->text_len = text_len;
    b->props_len = props_len;
    bool ok = batch_alloc(b) == hipSuccess;
    if (ok) {
        ok = hipMemcpy(b->off, doc_op_off, (h->n_docs + 1) * sizeof(int64_t), hipMemcpyHostToDevice) == hipSuccess;
        if (ok && n_ops) ok = hipMemcpy(b->ops, ops, n_ops * sizeof(mt_op_rec), hipMemcpyHostToDevice) == hipSuccess;
        if (ok && text_len) ok = hipMemcpy(b->text, text, text_len * 2, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && props_len) ok = hipMemcpy(b->props, props, props_len * 4, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) ok = set_order(b, doc_op_off);
    }
    if (!ok) {
        h->err = "mt_batch_upload: device allocation/copy failed";
        mt_batch_free(b);
        return nullptr;
    }
    return b;
}

// documents in the big region that this batch's LDS tier flagged (retry 1) skip the tight and
// full launches: the growth step replays them at the big region's capacities (retry 3)
__global__ void k_mark_big(DevState st, const int64_t *off, int resume_set) {
    const int doc = blockIdx.x * blockDim.x + threadIdx.x;
    if (doc >= st.n_docs || st.bslot[doc] < 0 || st.retry[doc] != 1) return;
    st.retry[doc] = 3;
    if (!resume_set) st.resume[doc] = off[doc];
    atomicAdd(st.stats + 13, 1u);
}
// One paged launch over every document (those not at stage pc.stage exit at once); big: the
// documents of the big region (the growth step's launches).
static int launch_paged(mt_handle *h, const mt_batch *b, PagedCaps pc, int res, PagedSlice sl, bool big = false) {
    const Pick p = pick_paged(K_REPLAY_PAGED, facts(h), pc, big, 0);
    void *a[] = {&h->st, (void *)&b->ops, (void *)&b->off, (void *)&b->text, (void *)&b->props, &res, &pc, &sl};
    HIPCHK(h, launch_variant(p, h->n_docs, h->stream, a));
    return 0;
}

int mt_batch_apply_async(mt_handle *h, const mt_batch *b) {
    if (!h || !b || b->n_docs != h->n_docs) return MT_E_INVALID;
    if (h->pending) {   // the previous batch's growth step runs before anything else
        const int rc = mt_settle(h);
        if (rc) return rc;
    }
    h->st.order = b->order;   // (its launches and its growth step's)
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->st.stats, 0, MT_STATS_WORDS * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    if (h->lds.S > 0) {
        // LDS tier for every document; the ones that outgrow it are flagged and replayed
        // from HBM by the second launch (whose other workgroups exit at once)
        HIPCHK(h, launch_replay(pick_flat(K_REPLAY, facts(h), h->lds, 0), h, b, h->lds));
    } else {
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->st.retry, 1, h->n_docs, h->stream));
    }
    if (h->st.PP > 0) {
        // documents that outgrew the LDS tier continue in the paged layout: the tight tier
        // first (when configured), then the full capacities for the documents it handed over
        const int use_resume = h->lds.S > 0 ? 1 : 0;
        if (h->n_big > 0) {   // documents of the big region go straight to the growth step's launch
            hipLaunchKernelGGL(k_mark_big, dim3((h->n_docs + 255) / 256), dim3(256), 0, h->stream, h->st, b->off,
                               use_resume);
            HIPCHK(h, hipGetLastError());
        }
        const PagedCaps *tiers[2] = {h->pg_tight.PP ? &h->pg_tight : nullptr, &h->pg_full};
        const int n = (int)h->n_docs;
        for (const PagedCaps *pc : tiers) {
            if (!pc) continue;
            const int res = pc->stage == 2 ? 1 : use_resume;
            // the launches of this tier: one over every document, or (paged_slices, first
            // tier) m slices each leaving out a window of the r = n mod resident left-over
            // documents -- every launch is then whole rounds -- and a last one without limits
            std::vector<PagedSlice> sls;
            const int S = h->pg_resident, m = h->paged_slices;
            const int r = S > 0 ? n % S : 0;
            if (pc == tiers[0] && m > 1 && S > 0 && n > S && r > 0 && (int64_t)m * r <= n) {
                const int64_t q = ((int64_t)b->n_ops / n + m - 1) / m;
                for (int j = 0; j < m; j++) {
                    PagedSlice sl{q, j * r, (j + 1) * r, 0, 0};
                    if (j == 0) sl.cnt_lo = r, sl.cnt_hi = n;   // counted once: window 0 in launch 1
                    if (j == 1) sl.cnt_lo = 0, sl.cnt_hi = r;
                    sls.push_back(sl);
                }
                sls.push_back(PagedSlice{0, 0, 0, 0, 0});
            } else {
                sls.push_back(PagedSlice{0, 0, 0, 0, n});
            }
            // a sliced tier resumes every launch after its first from resume[doc]; without
            // the LDS tier nothing has written it yet, so seed it with each document's first
            // message and resume from the first launch on (a slice must never restart at off)
            int res_k = res;
            if (sls.size() > 1 && !res) {
                HIPCHK(h, hipMemcpyAsync(h->st.resume, b->off, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice,
                                         h->stream));
                res_k = 1;
            }
            PagedCaps pcx = *pc;   // a wide tight tier packs its table when every client id fits 8 bits
            pcx.packed = pc->tight && !pc->narrow && h->max_cli <= 127 && pc->PP <= 255 ? 1 : 0;   // (8-bit pages)
            for (const PagedSlice &sl : sls) {
                const int rc = launch_paged(h, b, pcx, res_k, sl, false);
                if (rc) return rc;
            }
        }
    } else {   // the HBM tier: a live handle's hands documents that could outgrow it to the live growth step
        const TierCaps caps = h->live ? live_caps(h) : glb_caps(h);
        HIPCHK(h, launch_replay(pick_flat(K_REPLAY, facts(h), caps, 0), h, b, caps));
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    if (h->st.PP > 0 || h->live) {   // its last paged / live tier may hand documents to a growth step
        h->pending = const_cast<mt_batch *>(b);
        h->pending->owner = h;
    }
    return 0;
}

uint64_t mt_batch_num_ops(const mt_batch *b) { return b ? b->n_ops : 0; }

// ---------------------------------------------------------------- growth step
// The paged capacities of mt_options (page_capacity, unsettled_capacity, page_heap_capacity)
// are a starting point, not a limit.  The last paged tier (PagedCaps.grow) hands a document
// that does not fit it at load, or whose next message could outgrow it (pg_room), to this
// step with the message index (retry = 3); mt_settle then moves every such document into
// the *big region* -- a second set of paged arrays whose capacities are doubled where the
// documents ran out (bounded by the 160 KiB a paged launch may stage in LDS) -- and replays
// the rest of their messages there, round after round, before anything else runs on the
// stream.  Only documents beyond the handle's sizing pay for it; the others never move.
struct MigItem {
    int32_t doc, src, dst;   // src: slot in the old big region (-1: the main arrays)
};
__global__ void __launch_bounds__(MT_WAVE) k_migrate_paged(DevState st, PagedRegion old_big, PagedRegion dst_r,
                                                           const MigItem *items) {
    const MigItem it = items[blockIdx.x];
    const DocHdr h = st.hdr[it.doc];
    const PagedBase s = it.src < 0 ? paged_base(main_region(st), (size_t)it.doc) : paged_base(old_big, (size_t)it.src);
    const PagedBase d = paged_base(dst_r, (size_t)it.dst);
    {   // the live half of the text / property arenas (same half, same offsets): every record
        // below text_top / props_top
        const uint16_t *ts = s.text + (size_t)h.text_half * s.T;
        uint16_t *td = d.text + (size_t)h.text_half * d.T;
        for (int i = lane(); i < h.text_top; i += MT_WAVE) td[i] = ts[i];
        const uint32_t *ps = s.props + (size_t)h.props_half * s.P * MT_PREC;
        uint32_t *pd = d.props + (size_t)h.props_half * d.P * MT_PREC;
        for (size_t i = lane(); i < (size_t)h.props_top * MT_PREC; i += MT_WAVE) pd[i] = ps[i];
        // the uid map's entries below next_uid (a flat document has none yet)
        if (h.pad[HDR_PAGED])
            for (int i = lane(); i < min(h.next_uid, s.UM); i += MT_WAVE) d.umap[i] = s.umap[i];
        // the overflow overlap arena up to its fill (sets keep their offsets)
        if (s.ovf && d.ovf) {
            const int top = min(max((int)((const uint32_t *)s.ovf)[0], MT_OVF_HDR), s.OA);
            for (int i = lane(); i < top; i += MT_WAVE) d.ovf[i] = s.ovf[i];
        }
    }
    if (!h.pad[HDR_PAGED]) return;   // still flat: pg_convert pages it at the new capacities
    const size_t ns = (size_t)s.PP * MT_PG_SLOTS;   // page p slot k sits at p * 64 + k in both
    for (size_t i = lane(); i < ns; i += MT_WAVE) {
        d.A[i] = s.A[i];
        d.O[i] = s.O[i];
        d.B[i] = s.B[i];
    }
    for (int i = lane(); i < s.PP; i += MT_WAVE) {
        d.meta[i] = s.meta[i];
        d.dir[i] = s.dir[i];
    }
    for (int l = 0; l < MT_LV; l++)
        for (int b = lane(); b < s.PP; b += MT_WAVE) d.cnt[(size_t)l * d.PP + b] = s.cnt[(size_t)l * s.PP + b];
    for (int i = lane(); i <= s.PH; i += MT_WAVE) d.heap[i] = s.heap[i];
    for (int i = lane(); i < s.UT; i += MT_WAVE) {
        d.upage[i] = s.upage[i];
        d.uA[i] = s.uA[i];
        d.uO[i] = s.uO[i];
    }
    if (s.oS && d.oS) {   // segment ordinals: per page (same page ids), levels by position
        for (size_t i = lane(); i < ns; i += MT_WAVE) d.oS[i] = s.oS[i];
        for (size_t i = lane(); i < (size_t)s.PP * MT_PG_OLB; i += MT_WAVE) d.oL[i] = s.oL[i];
        for (int l = 0; l < MT_LV; l++)
            for (int b = lane(); b < s.PP; b += MT_WAVE) d.oU[(size_t)l * d.PP + b] = s.oU[(size_t)l * s.PP + b];
    }
}
// documents the growth step cannot serve (out of device memory) fail as before the step existed
__global__ void k_fail_grow(DevState st) {
    const int doc = blockIdx.x * blockDim.x + threadIdx.x;
    if (doc >= st.n_docs || st.retry[doc] != 3) return;
    st.retry[doc] = 0;
    if (st.hdr[doc].status == 0) {
        st.hdr[doc].status = MT_DOC_CAPACITY;
        st.hdr[doc].pad[HDR_DIAG] = 12;
    }
}

static bool alloc_region(PagedRegion &R, int slots, const PagedCaps &c, bool ordinals, int T, int P, int UM, int OA) {
    R = PagedRegion{};
    R.PP = c.PP;
    R.PH = c.PH;
    R.UT = c.UT;
    R.T = T;
    R.P = P;
    R.UM = UM;
    R.OA = OA;
    R.slots = slots;
    const size_t n = (size_t)slots, pages = n * c.PP;
    bool ok = hipMalloc(&R.A, pages * MT_PG_SLOTS * sizeof(int4)) == hipSuccess &&
              hipMalloc(&R.O, pages * MT_PG_SLOTS * sizeof(u64)) == hipSuccess &&
              hipMalloc(&R.B, pages * MT_PG_SLOTS * sizeof(uint4)) == hipSuccess &&
              hipMalloc(&R.meta, pages * sizeof(PageMeta)) == hipSuccess &&
              hipMalloc(&R.dir, pages * sizeof(uint16_t)) == hipSuccess &&
              hipMalloc(&R.cnt, pages * MT_LV) == hipSuccess &&
              hipMalloc(&R.heap, n * (size_t)(c.PH + 1) * sizeof(int2)) == hipSuccess &&
              hipMalloc(&R.upage, n * (size_t)c.UT * sizeof(int32_t)) == hipSuccess &&
              hipMalloc(&R.uA, n * (size_t)c.UT * sizeof(int4)) == hipSuccess &&
              hipMalloc(&R.uO, n * (size_t)c.UT * sizeof(u64)) == hipSuccess &&
              hipMalloc(&R.text, n * 2 * (size_t)T * sizeof(uint16_t)) == hipSuccess &&
              hipMalloc(&R.props, n * 2 * (size_t)P * MT_PREC * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc(&R.umap, n * (size_t)UM * sizeof(uint16_t)) == hipSuccess &&
              hipMalloc(&R.ovf, n * (size_t)OA * sizeof(uint16_t)) == hipSuccess &&
              hipMemset(R.ovf, 0, n * (size_t)OA * sizeof(uint16_t)) == hipSuccess;
    if (ok && ordinals)
        ok = hipMalloc(&R.oS, pages * MT_PG_SLOTS * sizeof(uint16_t)) == hipSuccess &&
             hipMalloc(&R.oL, pages * MT_PG_OLB * sizeof(uint16_t)) == hipSuccess &&
             hipMalloc(&R.oU, pages * MT_LV * sizeof(uint16_t)) == hipSuccess;
    if (!ok) free_region(R);
    return ok;
}


// Moves the documents of `moving` (and every document already there) into a new big region at
// capacities c, text / property arenas of T units / P records per half, UM uid-map entries
// and OA overflow-arena units; synchronous.
static int regrow(mt_handle *h, const std::vector<uint32_t> &moving, const PagedCaps &c, int T, int P, int UM,
                  int OA) {
    DevState &st = h->st;
    const uint32_t n = h->n_docs;
    if (!st.bslot) {
        HIPCHK(h, hipMalloc(&st.bslot, (size_t)n * sizeof(int32_t)));
        HIPCHK(h, hipMemset(st.bslot, 0xFF, (size_t)n * sizeof(int32_t)));
        h->bslot_h.assign(n, -1);
    }
    std::vector<int32_t> nb(n, -1);
    std::vector<MigItem> items;
    std::vector<uint8_t> mv(n, 0);
    for (uint32_t d : moving) mv[d] = 1;
    int slots = 0;
    for (uint32_t d = 0; d < n; d++)
        if (h->bslot_h[d] >= 0 || mv[d]) {
            nb[d] = slots;
            items.push_back(MigItem{(int32_t)d, h->bslot_h[d], slots});
            slots++;
        }
    struct NewRegion {   // freed unless it is installed as st.big
        PagedRegion R{};
        ~NewRegion() { free_region(R); }
    } nr;
    if (!alloc_region(nr.R, std::max(slots, 1), c, h->ordinals, T, P, UM, OA)) {
        (void)hipGetLastError();
        h->err = "growth step: device allocation of the big region failed";
        return MT_E_NOMEM;
    }
    DevBuf<MigItem> d_items;
    if (d_items.alloc(items.size()) != hipSuccess) return MT_E_NOMEM;
    HIPCHK(h, hipMemcpy(d_items.p, items.data(), items.size() * sizeof(MigItem), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_migrate_paged, dim3((uint32_t)items.size()), dim3(MT_WAVE), 0, h->stream, st, st.big, nr.R,
                       (const MigItem *)d_items.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(st.bslot, nb.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    free_region(st.big);
    st.big = nr.R;
    nr.R = PagedRegion{};
    h->bslot_h = nb;
    h->n_big = (uint32_t)slots;
    h->big_caps = PagedCaps{c.PP, c.PH, c.UT, 0, 3, 0, 1};
    return 0;
}

// The growth step's next capacities (grow_loop for replayed documents, load_grow for staged
// summary headers): c doubled where the documents ran out (t: the unsettled table, hp: the
// heap, pg: the pages), one capacity at a time while one paged launch can stage the layout in LDS
static PagedCaps grown_caps(const PagedCaps &c, bool t, bool hp, bool pg) {
    auto fits = [](const PagedCaps &q) { return paged_layout(q.PP, q.PH, q.UT, 0, 8).total <= 160 * 1024; };
    PagedCaps r = c, x = c;
    if (t) x.UT = std::min(2 * x.UT, 1 << 20);
    if (fits(x)) r = x;
    x = r;
    if (hp) x.PH = std::min(2 * x.PH, 1 << 20);
    if (fits(x)) r = x;
    x = r;
    if (pg) x.PP = std::min(2 * x.PP, 65535);
    if (fits(x)) r = x;
    return r;
}
// ... never below the big region's, once there is one: its paged capacities, arenas (T, P), uid
// map (U) and overflow arena (O)
static void at_least_big(const mt_handle *h, PagedCaps &c, int &T, int &P, int &U, int &O) {
    if (h->big_caps.PP <= 0) return;
    c.PP = std::max(c.PP, h->big_caps.PP);
    c.PH = std::max(c.PH, h->big_caps.PH);
    c.UT = std::max(c.UT, h->big_caps.UT);
    T = std::max(T, h->st.big.T);
    P = std::max(P, h->st.big.P);
    U = std::max(U, h->st.big.UM);
    O = std::max(O, h->st.big.OA);
}
static bool same_caps(const PagedCaps &a, const PagedCaps &b) { return a.PP == b.PP && a.PH == b.PH && a.UT == b.UT; }

// After the launches of batch b: re-tiers and replays the documents they handed to the
// growth step until none is left (synchronous).
static int grow_loop(mt_handle *h, const mt_batch *b) {
    DevState &st = h->st;
    st.order = b->order;
    const uint32_t n = h->n_docs;
    h->grown_last = 0;
    h->grow_rounds_last = 0;
    PagedCaps launched = h->pg_full;   // the capacities of the launch that handed them over
    bool launched_big = false;         // ... and whether it was the big region's launch
    std::vector<int32_t> retry(n);
    std::vector<DocHdr> hdr(n);
    for (int round = 0; round < 32; round++) {
        uint32_t g = 0;
        HIPCHK(h, hipMemcpy(&g, st.stats + 13, sizeof(g), hipMemcpyDeviceToHost));
        if (g == 0) return 0;
        HIPCHK(h, hipMemset(st.stats + 13, 0, sizeof(g)));
        HIPCHK(h, hipMemcpy(retry.data(), st.retry, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(hdr.data(), st.hdr, (size_t)n * sizeof(DocHdr), hipMemcpyDeviceToHost));
        std::vector<uint32_t> moving;
        // what ran out, read from the handed-over documents' state: a capacity they fill to
        // more than half is doubled (the kernel's bound is per message, pg_room); documents
        // of the big region marked for this batch (k_mark_big) only need its capacities
        bool t = false, hp = false, pg = false, tx = false, pr = false, um = false, ov = false;
        int judged = 0;
        for (uint32_t d = 0; d < n; d++) {
            if (retry[d] != 3) continue;
            moving.push_back(d);
            const bool in_big = !h->bslot_h.empty() && h->bslot_h[d] >= 0;
            if (in_big && !launched_big) continue;
            judged++;
            const DocHdr &x = hdr[d];
            const int np = x.pad[HDR_PAGED] ? x.pad[HDR_NPAGES] : (x.depth > 1 ? x.n_blk[1] : 1);
            t = t || 2 * x.pad[HDR_UTN] > launched.UT;
            hp = hp || 2 * x.heap_n > launched.PH;
            pg = pg || 2 * (np + 8) > launched.PP;
            if (x.pad[HDR_PAGED])   // an upper level near its room (pcnt_cap scales with the pages)
                for (int l = 2; l < x.depth && l < MT_LV; l++) pg = pg || 2 * (x.n_blk[l] + 4) > pcnt_cap(launched.PP, l);
            const int cause = x.status == 0 ? x.pad[HDR_DIAG] : 0;   // an arena hand-over (pg_arena_room)
            tx = tx || cause == 4;
            pr = pr || cause == 5;
            um = um || cause == 9;
            ov = ov || cause == 11;
        }
        if (moving.empty()) return 0;
        if (!t && !hp && !pg && !tx && !pr && !um && !ov) t = hp = true;   // a single message's bound (a long range): its table / heap terms
        h->grown_last += (uint32_t)moving.size();
        h->grow_rounds_last++;
        // the new capacities: doubled where the documents ran out, never below the big
        // region's, within the LDS one paged launch may stage
        const bool have = h->big_caps.PP > 0;
        PagedCaps nc = judged ? grown_caps(launched, t, hp, pg) : h->big_caps;   // (judged == 0: only marked documents)
        // the text / property arenas and the uid map (HBM only): doubled when a document's live
        // text / records / segments fill more than half of them after a compaction
        const int lT = launched_big ? st.big.T : st.T, lP = launched_big ? st.big.P : st.P;
        const int lU = launched_big ? st.big.UM : st.UM, lO = launched_big ? st.big.OA : st.OA;
        int nT = judged && tx ? (int)std::min<int64_t>(2LL * lT, 1 << 28) : lT;
        int nP = judged && pr ? (int)std::min<int64_t>(2LL * lP, 1 << 26) : lP;
        int nU = judged && um ? (int)std::min<int64_t>(2LL * lU, 1 << 24) : lU;
        int nO = judged && ov ? (int)std::min<int64_t>(2LL * lO, 1 << 30) : lO;
        at_least_big(h, nc, nT, nP, nU, nO);
        int rc = 0;
        PagedCaps pc = nc;
        bool big = true;
        if (same_caps(nc, launched) && nT == lT && nP == lP && nU == lU && nO == lO) {
            // no LDS capacity can grow: the documents run to their end at the capacities they
            // were handed over at (in their own region) and fail as before the step existed
            // only if they do outgrow them -- the arenas and the uid map still grow
            pc = launched;
            pc.grow = 2;
            big = launched_big;
        } else {
            bool all_big = have;
            for (uint32_t d : moving) all_big = all_big && !h->bslot_h.empty() && h->bslot_h[d] >= 0;
            if (!(all_big && same_caps(nc, h->big_caps) && nT == st.big.T && nP == st.big.P && nU == st.big.UM &&
                  nO == st.big.OA))
                rc = regrow(h, moving, nc, nT, nP, nU, nO);
            pc.grow = 1;   // (the arenas can always grow; a round that raises nothing runs with grow 0)
        }
        if (rc) {
            hipLaunchKernelGGL(k_fail_grow, dim3((n + 255) / 256), dim3(256), 0, h->stream, st);
            HIPCHK(h, hipStreamSynchronize(h->stream));
            return rc;
        }
        pc.tight = 0;
        pc.stage = 3;
        pc.narrow = 0;
        rc = launch_paged(h, b, pc, 1, PagedSlice{0, 0, 0, 0, 0}, big);
        if (rc) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        launched = pc;
        launched_big = big;
    }
    h->err = "growth step: no progress after 32 rounds";
    return MT_E_HIP;
}

// ---------------------------------------------------------------- live growth step
// Live (participant) documents replay on the flat HBM tier, whose per-document capacities
// (segments, blocks, heap, text and property arenas, segment groups) are the handle's.  They
// are a starting point, not a limit: a document whose next message could outgrow them
// (live_room) stops before it and is handed here; the step doubles what ran out for the whole
// handle -- every document's arrays are copied to the new strides (k_live_regrow) -- and
// replays the rest of the handed-over documents' messages, round after round.  Group ids are
// a ring of st.LG: growing it renumbers each document's outstanding groups from 1 (the
// segments' pending-group FIFOs with them).
struct LiveArrays {
    int32_t S, B, H, T, P, LG;
    int4 *segA;
    u64 *segO;
    uint4 *segB;
    uint8_t *cnt;
    int8_t *flg;
    int2 *heap;
    uint16_t *text;
    uint32_t *props;
    PendQ *segP;
    int32_t *grp;
    uint16_t *ordS, *ordB;
};
__global__ void __launch_bounds__(MT_WAVE) k_live_regrow(const DocHdr *hdr, int32_t *live, LiveArrays a, LiveArrays b) {
    const size_t doc = blockIdx.x;
    const DocHdr h = hdr[doc];
    const int n = h.n_seg;
    for (int i = lane(); i < n; i += MT_WAVE) {
        b.segA[doc * b.S + i] = a.segA[doc * a.S + i];
        b.segO[doc * b.S + i] = a.segO[doc * a.S + i];
        b.segB[doc * b.S + i] = a.segB[doc * a.S + i];
        if (a.ordS) b.ordS[doc * b.S + i] = a.ordS[doc * a.S + i];
    }
    for (int l = 0; l < MT_LV; l++)
        for (int q = lane(); q < h.n_blk[l]; q += MT_WAVE) {
            b.cnt[doc * MT_LV * b.B + (size_t)l * b.B + q] = a.cnt[doc * MT_LV * a.B + (size_t)l * a.B + q];
            if (a.ordB) b.ordB[doc * MT_LV * b.B + (size_t)l * b.B + q] = a.ordB[doc * MT_LV * a.B + (size_t)l * a.B + q];
        }
    for (int q = lane(); q < h.n_blk[0]; q += MT_WAVE) b.flg[doc * b.B + q] = a.flg[doc * a.B + q];
    for (int i = 1 + lane(); i <= h.heap_n; i += MT_WAVE) b.heap[doc * (b.H + 1) + i] = a.heap[doc * (a.H + 1) + i];
    {   // the live half of the arenas, same offsets
        const uint16_t *ts = a.text + doc * 2 * a.T + (size_t)h.text_half * a.T;
        uint16_t *td = b.text + doc * 2 * b.T + (size_t)h.text_half * b.T;
        for (int i = lane(); i < h.text_top; i += MT_WAVE) td[i] = ts[i];
        const uint32_t *ps = a.props + doc * 2 * a.P * MT_PREC + (size_t)h.props_half * a.P * MT_PREC;
        uint32_t *pd = b.props + doc * 2 * b.P * MT_PREC + (size_t)h.props_half * b.P * MT_PREC;
        for (size_t i = lane(); i < (size_t)h.props_top * MT_PREC; i += MT_WAVE) pd[i] = ps[i];
    }
    // segment groups: outstanding ids g_head .. (ring of a.LG) -> 1 .. g_n
    const int g_head = live[4 * doc + 1], g_n = live[4 * doc + 2];
    const bool renum = b.LG != a.LG;
    auto nid = [&](int x) { return x == 0 ? 0 : (renum ? (x - g_head + a.LG) % a.LG + 1 : x); };
    for (int i = lane(); i < n; i += MT_WAVE) {
        PendQ q = a.segP[doc * a.S + i];
        if (renum)
            for (int k = 0; k < 4; k++) {
                u64 w = 0;
                for (int j = 0; j < 4; j++) w |= (u64)(uint32_t)nid((int)((q.w[k] >> (16 * j)) & 0xFFFFull)) << (16 * j);
                q.w[k] = w;
            }
        b.segP[doc * b.S + i] = q;
    }
    const size_t ga = doc * (size_t)(a.LG + 1) * MT_GRP_WORDS, gb = doc * (size_t)(b.LG + 1) * MT_GRP_WORDS;
    if (!renum) {
        for (int i = lane(); i < (a.LG + 1) * MT_GRP_WORDS; i += MT_WAVE) b.grp[gb + i] = a.grp[ga + i];
    } else {
        for (int k = 0; k < g_n; k++) {
            const int x = (g_head - 1 + k) % a.LG + 1;
            if (lane() < MT_GRP_WORDS)
                b.grp[gb + (size_t)(k + 1) * MT_GRP_WORDS + lane()] = a.grp[ga + (size_t)x * MT_GRP_WORDS + lane()];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane() == 0) live[4 * doc + 1] = 1;
    }
}
static LiveArrays live_arrays(const DevState &st) {
    return LiveArrays{st.S, st.B, st.H, st.T, st.P, st.LG, (int4 *)st.segA, (u64 *)st.segO, (uint4 *)st.segB,
                      (uint8_t *)st.cnt, (int8_t *)st.flg, (int2 *)st.heap, (uint16_t *)st.text, (uint32_t *)st.props,
                      (PendQ *)st.segP, (int32_t *)st.grp, (uint16_t *)st.ordS, (uint16_t *)st.ordB};
}
// every document's flat arrays at the new capacities
static int live_regrow(mt_handle *h, int S2, int B2, int H2, int T2, int P2, int LG2) {
    DevState &st = h->st;
    const size_t N = h->n_docs;
    LiveArrays a = live_arrays(st), b = a;
    b.S = S2, b.B = B2, b.H = H2, b.T = T2, b.P = P2, b.LG = LG2;
    bool ok = true;
    auto alloc = [&](auto **p, size_t bytes) {
        *p = nullptr;
        if (ok && hipMalloc((void **)p, bytes ? bytes : 16) != hipSuccess) ok = false;
    };
    alloc(&b.segA, N * S2 * sizeof(int4));
    alloc(&b.segO, N * S2 * sizeof(u64));
    alloc(&b.segB, N * S2 * sizeof(uint4));
    alloc(&b.cnt, N * MT_LV * (size_t)B2);
    alloc(&b.flg, N * (size_t)B2);
    alloc(&b.heap, N * (size_t)(H2 + 1) * sizeof(int2));
    alloc(&b.text, N * 2 * (size_t)T2 * sizeof(uint16_t));
    alloc(&b.props, N * 2 * (size_t)P2 * MT_PREC * sizeof(uint32_t));
    alloc(&b.segP, N * (size_t)S2 * sizeof(PendQ));
    alloc(&b.grp, N * (size_t)(LG2 + 1) * MT_GRP_WORDS * sizeof(int32_t));
    if (a.ordS) {
        alloc(&b.ordS, N * (size_t)S2 * sizeof(uint16_t));
        alloc(&b.ordB, N * (size_t)MT_LV * B2 * sizeof(uint16_t));
    }
    void *nb[] = {b.segA, b.segO, b.segB, b.cnt, b.flg, b.heap, b.text, b.props, b.segP, b.grp, b.ordS, b.ordB};
    if (!ok) {
        for (void *p : nb)
            if (p) hipFree(p);
        h->err = "live growth step: device allocation failed (HBM exhausted)";
        return MT_E_HIP;
    }
    hipLaunchKernelGGL(k_live_regrow, dim3((unsigned)N), dim3(MT_WAVE), 0, h->stream, st.hdr, st.live, a, b);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    void *old[] = {a.segA, a.segO, a.segB, a.cnt, a.flg, a.heap, a.text, a.props, a.segP, a.grp, a.ordS, a.ordB};
    for (void *p : old)
        if (p) hipFree(p);
    st.S = S2, st.B = B2, st.H = H2, st.T = T2, st.P = P2, st.LG = LG2;
    st.segA = (decltype(st.segA))b.segA;
    st.segO = (decltype(st.segO))b.segO;
    st.segB = (decltype(st.segB))b.segB;
    st.cnt = (decltype(st.cnt))b.cnt;
    st.flg = (decltype(st.flg))b.flg;
    st.heap = (decltype(st.heap))b.heap;
    st.text = (decltype(st.text))b.text;
    st.props = (decltype(st.props))b.props;
    st.segP = (decltype(st.segP))b.segP;
    st.grp = (decltype(st.grp))b.grp;
    st.ordS = (decltype(st.ordS))b.ordS;
    st.ordB = (decltype(st.ordB))b.ordB;
    return 0;
}
__global__ void k_live_fail_flagged(DevState st, int cause) {
    const int doc = blockIdx.x * blockDim.x + threadIdx.x;
    if (doc >= st.n_docs || !st.retry[doc]) return;
    st.retry[doc] = 0;
    st.hdr[doc].status = MT_DOC_CAPACITY;
    st.hdr[doc].pad[HDR_DIAG] = cause;
}
static int live_grow_loop(mt_handle *h, const mt_batch *b) {
    DevState &st = h->st;
    st.order = b->order;
    h->grown_last = 0;
    h->grow_rounds_last = 0;
    for (int round = 0; round < 40; round++) {
        uint32_t s[2];
        HIPCHK(h, hipMemcpy(s, st.stats + 13, sizeof(s), hipMemcpyDeviceToHost));
        if (s[0] == 0) return 0;
        HIPCHK(h, hipMemset(st.stats + 13, 0, sizeof(s)));
        const uint32_t c = s[1];
        int S2 = st.S, B2 = st.B, H2 = st.H, T2 = st.T, P2 = st.P, LG2 = st.LG;
        if (c & (1u << 1)) S2 = 2 * st.S;
        B2 = std::max(st.B * ((c & (1u << 2)) ? 2 : 1), (std::max(64, S2 / 2) + 63) / 64 * 64);
        H2 = std::max(st.H * ((c & (1u << 3)) ? 2 : 1), (int)((int64_t)st.H * S2 / st.S));
        if (c & (1u << 4)) T2 = 2 * st.T;
        P2 = std::max(st.P * ((c & (1u << 5)) ? 2 : 1), st.P + (S2 - st.S));
        if (c & (1u << 12)) LG2 = std::min(2 * st.LG, 65535);
        if (S2 == st.S && B2 == st.B && H2 == st.H && T2 == st.T && P2 == st.P && LG2 == st.LG) {
            // nothing left to grow (group ids are 16 bits): the documents fail as before
            hipLaunchKernelGGL(k_live_fail_flagged, dim3((h->n_docs + 255) / 256), dim3(256), 0, h->stream, st, 12);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipStreamSynchronize(h->stream));
            return 0;
        }
        const int rc = live_regrow(h, S2, B2, H2, T2, P2, LG2);
        if (rc) return rc;
        h->grown_last += s[0];
        h->grow_rounds_last++;
        TierCaps caps = glb_caps(h);
        caps.resume = 1;
        caps.grow = 1;
        HIPCHK(h, launch_replay(pick_flat(K_REPLAY, facts(h), caps, 0), h, b, caps));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->err = "live growth step: no progress after 40 rounds";
    return MT_E_HIP;
}

// Waits for the stream, then runs the growth step of the last applied batch.
static int mt_settle(mt_handle *h) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!h->pending) return 0;
    mt_batch *b = h->pending;
    h->pending = nullptr;
    const int rc = h->live ? live_grow_loop(h, b) : grow_loop(h, b);
    b->owner = nullptr;
    // the growth step's launches belong to the batch: the batch's timing (mt_last_kernel_ms)
    // ends after them
    if (h->grown_last > 0 && h->timed) {
        HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        HIPCHK(h, hipEventSynchronize(h->ev1));
    }
    return rc;
}

void mt_batch_free(mt_batch *b) {
    if (!b) return;
    if (b->owner && b->owner->pending == b) mt_settle(b->owner);   // its growth step still reads it
    hipSetDevice(b->device);
    if (b->off) hipFree(b->off);
    if (b->ops) hipFree(b->ops);
    if (b->text) hipFree(b->text);
    if (b->props) hipFree(b->props);
    if (b->order) hipFree(b->order);
    delete b;
}

void *mt_host_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void mt_host_free(void *p) {
    if (p) hipHostFree(p);
}

int mt_sync(mt_handle *h) {
    if (!h) return MT_E_INVALID;
    const int rc = mt_settle(h);
    if (rc) return rc;
    if (h->timed) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_ms = ms;
        (void)hipGetLastError();   // never leave a sticky error for the next launch check
        h->timed = false;
    }
    return 0;
}

float mt_last_kernel_ms(const mt_handle *h) { return h ? h->last_ms : 0.f; }

// The handle's stream again, at a scheduling priority: > 0 the device's highest, < 0 its
// lowest, 0 the default.  Handles sharing the GPU (the skewed bench's size classes, each on its
// own stream) dispatch the high-priority stream's waiting workgroups first as CUs free up.
int mt_set_stream_priority(mt_handle *h, int priority) {
    if (!h) return MT_E_INVALID;
    const int rc = mt_sync(h);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int least = 0, greatest = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t s = nullptr;
    HIPCHK(h, hipStreamCreateWithPriority(&s, hipStreamNonBlocking,
                                          priority > 0 ? greatest : (priority < 0 ? least : 0)));
    hipStreamDestroy(h->stream);
    h->stream = s;
    return 0;
}

int mt_last_hbm_docs(mt_handle *h, uint32_t *out) {
    if (!h || !out) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    HIPCHK(h, hipMemcpy(out, h->st.stats, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mt_last_grown(mt_handle *h, uint32_t *out) {
    if (!h || !out) return MT_E_INVALID;
    SETTLE(h);
    uint32_t in_big = 0;
    for (int32_t x : h->bslot_h) in_big += x >= 0;
    out[0] = h->grown_last;
    out[1] = h->grow_rounds_last;
    out[2] = in_big;
    out[3] = (uint32_t)h->big_caps.PP;
    out[4] = (uint32_t)h->big_caps.UT;
    out[5] = (uint32_t)h->big_caps.PH;
    return 0;
}

int mt_last_paged_peaks(mt_handle *h, uint32_t *out) {
    if (!h || !out) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    HIPCHK(h, hipMemcpy(out, h->st.stats + 8, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mt_last_zamboni(mt_handle *h, uint32_t *out) {
    if (!h || !out) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    HIPCHK(h, hipMemcpy(out, h->st.stats + 16, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mt_last_zamboni_packs(mt_handle *h, uint32_t *out) {
    if (!h || !out) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    HIPCHK(h, hipMemcpy(out, h->st.stats + 18, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mt_last_range_paths(mt_handle *h, uint32_t *out) {
    if (!h || !out) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    HIPCHK(h, hipMemcpy(out, h->st.stats + 20, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    out[0] -= out[1];   // the device counts entries into the path; those that left it are out[1]
    return 0;
}

int mt_apply_ops(mt_handle *h, const int64_t *doc_op_off, const mt_op_rec *ops, uint64_t n_ops,
                 const uint16_t *text, uint64_t text_len, const uint32_t *props,
                 uint64_t props_len) {
    if (!h) return MT_E_INVALID;
    h->err.clear();
    mt_batch *b = mt_batch_upload(h, doc_op_off, ops, n_ops, text, text_len, props, props_len);
    if (!b) return h->err.rfind("mt_batch_upload: device", 0) == 0 ? MT_E_NOMEM : MT_E_INVALID;
    int rc = mt_batch_apply_async(h, b);
    if (rc == 0) rc = mt_sync(h);
    mt_batch_free(b);
    return rc;
}

struct mt_snapshots {
    int device = 0;
    uint32_t doc_lo = 0, n_docs = 0;   // summary d loads into document doc_lo + d
    int64_t *off = nullptr;
    int32_t *nh = nullptr, *min_seq = nullptr, *cur_seq = nullptr;
    mt_seg_rec *segs = nullptr;
    uint16_t *text = nullptr;
    uint32_t *props = nullptr;
    mt_batch *body = nullptr;   // loadBody appends as MT_F_LOAD records (nullptr: none)
    // headers larger than the flat capacities on a paged handle (k_load_convert)
    LoadScratch sc = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t *sc_off = nullptr;
    std::vector<int64_t> sc_off_h;   // host copy of sc_off (load_grow)
    bool any_big = false;
};

void mt_snapshots_free(mt_snapshots *s) {
    if (!s) return;
    hipSetDevice(s->device);
    void *ps[] = {s->off, s->nh, s->min_seq, s->cur_seq, s->segs, s->text, s->props, s->sc.A, s->sc.O, s->sc.B,
                  s->sc.cnt, s->sc.flg, s->sc_off};
    for (void *p : ps)
        if (p) hipFree(p);
    mt_batch_free(s->body);
    delete s;
}

mt_snapshots *mt_snapshots_upload_range(mt_handle *h, uint32_t doc_lo, uint32_t n_docs, const int64_t *doc_seg_off,
                                        const int32_t *n_header, const mt_seg_rec *segs, uint64_t n_segs,
                                        const uint16_t *text, uint64_t text_len, const uint32_t *props,
                                        uint64_t props_len, const int32_t *min_seq, const int32_t *cur_seq) {
    if (!h || !doc_seg_off || !n_header || !min_seq || !cur_seq || (n_segs && !segs)) return nullptr;
    if (n_docs == 0 || doc_lo > h->n_docs || n_docs > h->n_docs - doc_lo) {
        h->err = "mt_snapshots_upload_range: documents [doc_lo, doc_lo + n_docs) outside the handle (or empty)";
        return nullptr;
    }
    const uint32_t N = n_docs;   // summary d of this set loads into document doc_lo + d
    for (uint32_t d = 0; d < N; d++)
        if (n_header[d] < 0 || doc_seg_off[d] + n_header[d] > doc_seg_off[d + 1] ||
            doc_seg_off[d + 1] > (int64_t)n_segs) {
            h->err = "mt_snapshots_upload: bad document segment ranges";
            return nullptr;
        }
    for (uint64_t i = 0; i < (uint64_t)doc_seg_off[N]; i++) {
        const mt_seg_rec &r = segs[i];
        h->max_cli = std::max({h->max_cli, std::abs((int)r.client), std::abs((int)r.removed_client)});
        const bool marker = (r.flags & MT_F_MARKER) != 0;
        if (r.len < 0 || (!marker && (uint64_t)r.payload + (uint64_t)r.len > text_len) ||
            !props_rec_ok(props, props_len, r.props)) {
            h->err = "mt_snapshots_upload: segment record " + std::to_string(i) + " outside the arenas";
            return nullptr;
        }
    }
    if (hipSetDevice(h->device) != hipSuccess) return nullptr;
    auto *s = new mt_snapshots();
    s->device = h->device;
    s->n_docs = N;
    s->doc_lo = doc_lo;
    bool ok = hipMalloc(&s->off, (N + 1) * 8) == hipSuccess && hipMalloc(&s->nh, N * 4) == hipSuccess &&
              hipMalloc(&s->min_seq, N * 4) == hipSuccess && hipMalloc(&s->cur_seq, N * 4) == hipSuccess &&
              hipMalloc(&s->segs, std::max<uint64_t>(n_segs, 1) * sizeof(mt_seg_rec)) == hipSuccess &&
              hipMalloc(&s->text, std::max<uint64_t>(text_len, 1) * 2) == hipSuccess &&
              hipMalloc(&s->props, std::max<uint64_t>(props_len, 1) * 4) == hipSuccess;
    ok = ok && hipMemcpy(s->off, doc_seg_off, (N + 1) * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s->nh, n_header, N * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s->min_seq, min_seq, N * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s->cur_seq, cur_seq, N * 4, hipMemcpyHostToDevice) == hipSuccess &&
         (!n_segs || hipMemcpy(s->segs, segs, n_segs * sizeof(mt_seg_rec), hipMemcpyHostToDevice) == hipSuccess) &&
         (!text_len || hipMemcpy(s->text, text, text_len * 2, hipMemcpyHostToDevice) == hipSuccess) &&
         (!props_len || hipMemcpy(s->props, props, props_len * 4, hipMemcpyHostToDevice) == hipSuccess);
    // a header beyond the flat capacities is staged and paged (handles with a paged layout)
    if (ok && h->st.PP > 0) {
        std::vector<int64_t> so((size_t)N * 2, -1);
        int64_t ns = 0, nb = 0;
        for (uint32_t d = 0; d < N; d++) {
            const int64_t n = n_header[d], nb0 = n > 0 ? (n + MT_LOAD_FANOUT - 1) / MT_LOAD_FANOUT : 1;
            if (n > h->st.S || nb0 > h->st.B) {
                so[2 * d] = ns;
                so[2 * d + 1] = nb;
                ns += n;
                nb += nb0;
            }
        }
        if (ns > 0) {
            s->any_big = true;
            ok = hipMalloc(&s->sc.A, ns * sizeof(int4)) == hipSuccess &&
                 hipMalloc(&s->sc.O, ns * sizeof(u64)) == hipSuccess &&
                 hipMalloc(&s->sc.B, ns * sizeof(uint4)) == hipSuccess &&
                 hipMalloc(&s->sc.cnt, (size_t)nb * MT_LV) == hipSuccess &&
                 hipMalloc(&s->sc.flg, (size_t)nb) == hipSuccess &&
                 hipMalloc(&s->sc_off, (size_t)N * 16) == hipSuccess &&
                 hipMemcpy(s->sc_off, so.data(), (size_t)N * 16, hipMemcpyHostToDevice) == hipSuccess;
            s->sc.off = s->sc_off;
            s->sc_off_h = so;
        }
    }
    if (!ok) {
        h->err = "mt_snapshots_upload: device allocation/copy failed";
        mt_snapshots_free(s);
        return nullptr;
    }
    // loadBody (MT/snapshotLoader.ts:161-228): specs without merge info (NonCollabClient,
    // seq 0) are appended in batches -- one insertSegments: one boundary at the batch start
    // (root.cachedLength), then each segment at insertPos += cachedLength -- the others one
    // by one at root.cachedLength.  Each append becomes an MT_F_LOAD insert record (refSeq
    // 0, the append's client and seq) plus MT_OP_LOAD_REMOVED when the spec carries removal
    // info; the ordinary replay kernels apply them (every tier).
    std::vector<mt_op_rec> ops;
    std::vector<int64_t> ooff(h->n_docs + 1, 0);   // the body batch spans the handle's documents
    for (uint32_t d = 0; d < N; d++) {
        ooff[doc_lo + d] = (int64_t)ops.size();
        const int64_t s0 = doc_seg_off[d], sh = s0 + n_header[d], s1 = doc_seg_off[d + 1];
        int64_t obs = 0;   // root.cachedLength: observer length (removed segments count 0)
        for (int64_t i = s0; i < sh; i++)
            if (segs[i].removed_seq == MT_RSEQ_NONE) obs += (segs[i].flags & MT_F_MARKER) ? 1 : segs[i].len;
        bool in_batch = false;
        int64_t ins = 0;
        // loadBody's batch is never emptied (:207-227): once it was flushed holding a segment
        // (of non-zero length -- blockInsert skips the others), the next flush (before the
        // next merge-info spec, or the final one) re-inserts it -> MT_DOC_ALIASED there
        bool batch_len = false, flushed = false, aliased = false;
        auto alias = [&]() {
            mt_op_rec q;
            memset(&q, 0, sizeof(q));
            q.kind = MT_OP_LOAD_ALIASED;
            q.flags = MT_F_LOAD;
            ops.push_back(q);
            aliased = true;
        };
        for (int64_t i = sh; i < s1 && !aliased; i++) {
            const mt_seg_rec &r = segs[i];
            const int len = (r.flags & MT_F_MARKER) ? 1 : r.len;
            const bool plain = r.client == -2 && r.seq == 0;
            const bool removed = r.removed_seq != MT_RSEQ_NONE;
            if (plain) {
                if (flushed) continue;   // inserted by the next flush, after the re-insertion
                if (!in_batch) ins = obs;
                in_batch = true;
                batch_len = batch_len || len > 0;
            } else {
                if (batch_len) {   // flushBatch() before this spec
                    if (flushed) {
                        alias();
                        break;
                    }
                    flushed = true;
                }
                in_batch = false;
                ins = obs;
            }
            if (len > 0) {   // blockInsert skips empty segments (:2229)
                mt_op_rec o;
                memset(&o, 0, sizeof(o));
                o.seq = plain ? 0 : r.seq;
                o.pos1 = (int32_t)ins;
                o.pos2 = len;
                o.payload = r.payload;
                o.props = r.props;
                o.client = (uint16_t)(plain ? -2 : r.client);
                o.kind = MT_OP_INSERT;
                o.flags = (uint8_t)(MT_F_LOAD | (r.flags & MT_F_MARKER));
                ops.push_back(o);
                if (removed) {
                    mt_op_rec q;
                    memset(&q, 0, sizeof(q));
                    q.seq = r.removed_seq;
                    q.client = (uint16_t)r.removed_client;
                    q.kind = MT_OP_LOAD_REMOVED;
                    q.flags = MT_F_LOAD;
                    ops.push_back(q);
                }
                ins += len;
            }
            if (!removed) obs += len;
        }
        if (!aliased && batch_len && flushed) alias();   // the final flushBatch()
    }
    for (uint32_t d = doc_lo + N; d <= h->n_docs; d++) ooff[d] = (int64_t)ops.size();
    if (!ops.empty()) {
        s->body = mt_batch_upload(h, ooff.data(), ops.data(), ops.size(), text, text_len, props, props_len);
        if (!s->body) {
            mt_snapshots_free(s);
            return nullptr;
        }
    }
    return s;
}

mt_snapshots *mt_snapshots_upload(mt_handle *h, const int64_t *doc_seg_off, const int32_t *n_header,
                                  const mt_seg_rec *segs, uint64_t n_segs, const uint16_t *text, uint64_t text_len,
                                  const uint32_t *props, uint64_t props_len, const int32_t *min_seq,
                                  const int32_t *cur_seq) {
    if (!h) return nullptr;
    return mt_snapshots_upload_range(h, 0, h->n_docs, doc_seg_off, n_header, segs, n_segs, text, text_len, props,
                                     props_len, min_seq, cur_seq);
}

// the staged headers of set s become paged documents at capacities pc (big: in the big region);
// a segment-ordinal handle's kernel derives the canonical ordinals (reloadFromSegments)
static hipError_t launch_load_convert(mt_handle *h, const mt_snapshots *s, PagedCaps pc, bool big) {
    LoadScratch sc = s->sc;
    int lo = (int)s->doc_lo;
    void *a[] = {&h->st, &sc, &pc, &lo};
    return launch_variant(pick_paged(K_LOAD_CONVERT, facts(h), pc, big, 0), s->n_docs, h->stream, a);
}
// A staged header that does not fit the paged capacities it was converted at (pages, the
// unsettled table: k_load_convert left it with MT_DOC_CAPACITY and the cause) is handed to the
// growth step's big region, as a replayed document that outgrows them is (grow_loop): what ran
// out is doubled, round after round, within the LDS one paged launch may stage, and
// k_load_convert's kBig instantiation pages the header there.  Synchronous; reached only by
// summary sets with staged headers.
static int load_grow(mt_handle *h, const mt_snapshots *s) {
    DevState &st = h->st;
    const uint32_t N = s->n_docs;
    std::vector<DocHdr> hdr(N);
    PagedCaps cur = h->pg_full;
    for (int round = 0; round < 16; round++) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(hdr.data(), st.hdr + s->doc_lo, (size_t)N * sizeof(DocHdr), hipMemcpyDeviceToHost));
        std::vector<uint32_t> moving;
        bool t = false, hp = false, pg = false;
        for (uint32_t r = 0; r < N; r++) {
            const DocHdr &x = hdr[r];
            if (s->sc_off_h[2 * r] < 0 || x.status != MT_DOC_CAPACITY || x.pad[HDR_PAGED]) continue;
            const int cause = x.pad[HDR_DIAG];
            if (cause != 3 && cause != 7 && cause != 8) continue;   // (an arena, the uid map: not the paged capacities)
            moving.push_back(s->doc_lo + r);
            t = t || cause == 8;
            hp = hp || cause == 3;
            pg = pg || cause == 7;
        }
        if (moving.empty()) return 0;
        PagedCaps nc = grown_caps(cur, t, hp, pg);
        if (same_caps(nc, cur)) return 0;   // nothing can grow: they stay failed
        int nT = st.T, nP = st.P, nU = st.UM, nO = st.OA;
        at_least_big(h, nc, nT, nP, nU, nO);
        const int rc = regrow(h, moving, nc, nT, nP, nU, nO);
        if (rc) return rc;
        for (uint32_t d : moving) {   // the header k_load_header wrote, without the failure
            DocHdr &xh = hdr[d - s->doc_lo];
            xh.status = 0;
            xh.pad[HDR_DIAG] = 0;
            HIPCHK(h, hipMemcpy(st.hdr + d, &xh, sizeof(DocHdr), hipMemcpyHostToDevice));
        }
        HIPCHK(h, launch_load_convert(h, s, h->big_caps, true));
        cur = nc;
    }
    return 0;
}

int mt_snapshots_load_async(mt_handle *h, const mt_snapshots *s) {
    if (!h || !s || s->doc_lo > h->n_docs || s->n_docs > h->n_docs - s->doc_lo) return MT_E_INVALID;
    if (h->pending) SETTLE(h);
    HIPCHK(h, hipSetDevice(h->device));
    if (h->n_big > 0) {   // loaded documents start over in the main arrays (k_load_header clears bslot)
        for (uint32_t d = s->doc_lo; d < s->doc_lo + s->n_docs; d++) {
            h->n_big -= h->bslot_h[d] >= 0;
            h->bslot_h[d] = -1;
        }
    }
    if (h->st.DL)
        HIPCHK(h, hipMemsetAsync(h->st.dlog + (size_t)s->doc_lo * h->st.DL, 0, (size_t)s->n_docs * h->st.DL * 4,
                                 h->stream));
    HIPCHK(h, hipEventRecord(h->ev_load, h->stream));
    hipLaunchKernelGGL(k_load_header, dim3(s->n_docs), dim3(MT_WAVE), 0, h->stream, h->st, s->off, s->nh, s->segs,
                       s->text, s->props, s->min_seq, s->cur_seq, s->sc, (int)s->doc_lo);
    HIPCHK(h, hipGetLastError());
    if (s->any_big) {
        HIPCHK(h, launch_load_convert(h, s, h->pg_full, false));
        const int rc = load_grow(h, s);
        if (rc) {   // (the load's events stay a pair: mt_last_load_ms reads both)
            (void)hipEventRecord(h->ev_load1, h->stream);
            h->load_timed = true;
            return rc;
        }
    }
    HIPCHK(h, hipEventRecord(h->ev_load1, h->stream));
    h->load_timed = true;
    if (s->body) return mt_batch_apply_async(h, s->body);
    return 0;
}

float mt_last_load_ms(mt_handle *h) {
    if (!h || !h->load_timed) return 0.f;
    float ms = 0.f;
    if (hipEventSynchronize(h->ev_load1) != hipSuccess || hipEventElapsedTime(&ms, h->ev_load, h->ev_load1) != hipSuccess)
        return 0.f;
    return ms;
}

int mt_load_snapshots(mt_handle *h, const int64_t *doc_seg_off, const int32_t *n_header, const mt_seg_rec *segs,
                      uint64_t n_segs, const uint16_t *text, uint64_t text_len, const uint32_t *props,
                      uint64_t props_len, const int32_t *min_seq, const int32_t *cur_seq) {
    if (!h) return MT_E_INVALID;
    if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return MT_E_HIP;
    mt_snapshots *s = mt_snapshots_upload(h, doc_seg_off, n_header, segs, n_segs, text, text_len, props, props_len,
                                          min_seq, cur_seq);
    if (!s) return MT_E_INVALID;
    int rc = mt_snapshots_load_async(h, s);
    if (rc == 0) rc = mt_sync(h);
    if (rc == 0 && hipStreamSynchronize(h->stream) != hipSuccess) rc = MT_E_HIP;
    mt_snapshots_free(s);
    return rc;
}

int mt_extract_snapshots(mt_handle *h, int64_t *io, mt_seg_rec *recs, uint16_t *text, uint32_t *props,
                         int32_t *min_seq, int32_t *cur_seq) {
    if (!h || !io) return MT_E_INVALID;
    const uint32_t N = h->n_docs;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    DevBuf<int64_t> d_io;
    HIPCHK(h, d_io.alloc((size_t)N * 3));
    const int mode = recs ? 1 : 0;
    uint64_t nr = 0, nt = 0, np = 0;
    std::vector<int64_t> off;
    if (mode) {   // io holds the counts of the first call: exclusive prefix sums
        off.resize((size_t)N * 3);
        for (uint32_t d = 0; d < N; d++) {
            off[3 * d] = (int64_t)nr;
            off[3 * d + 1] = (int64_t)nt;
            off[3 * d + 2] = (int64_t)np;
            nr += io[3 * d];
            nt += io[3 * d + 1];
            np += io[3 * d + 2];
        }
    }
    DevBuf<mt_seg_rec> d_recs;
    DevBuf<uint16_t> d_text;
    DevBuf<uint32_t> d_props;
    DevBuf<int32_t> d_win;
    HIPCHK(h, d_win.alloc((size_t)N * 2));
    if (mode) {
        HIPCHK(h, d_recs.alloc(nr));
        HIPCHK(h, d_text.alloc(nt));
        HIPCHK(h, d_props.alloc(np));
        HIPCHK(h, hipMemcpy(d_io.p, off.data(), (size_t)N * 3 * 8, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_extract, dim3(N), dim3(MT_WAVE), 0, h->stream, h->st, mode, d_io.p, d_recs.p, d_text.p,
                       d_props.p, d_win.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!mode) HIPCHK(h, hipMemcpy(io, d_io.p, (size_t)N * 3 * 8, hipMemcpyDeviceToHost));
    if (mode) {
        if (nr) HIPCHK(h, hipMemcpy(recs, d_recs.p, nr * sizeof(mt_seg_rec), hipMemcpyDeviceToHost));
        if (nt && text) HIPCHK(h, hipMemcpy(text, d_text.p, nt * 2, hipMemcpyDeviceToHost));
        if (np && props) HIPCHK(h, hipMemcpy(props, d_props.p, np * 4, hipMemcpyDeviceToHost));
    }
    std::vector<int32_t> win((size_t)N * 2);
    HIPCHK(h, hipMemcpy(win.data(), d_win.p, (size_t)N * 8, hipMemcpyDeviceToHost));
    for (uint32_t d = 0; d < N; d++) {
        if (min_seq) min_seq[d] = win[2 * d];
        if (cur_seq) cur_seq[d] = win[2 * d + 1];
    }
    return 0;
}

// Packs the generated documents' text / property regions (allocated at fixed strides) back
// to back and rebases their op records, whose offsets the generator wrote local to the
// document's region: the wire format's u32 offsets address the whole batch, and the strided
// layout would pass 2^32 units (C3: at document ~53.7k).
__global__ void __launch_bounds__(256) k_gen_compact(mt_op_rec *ops, const int64_t *off, const uint16_t *text_in,
                                                     const uint32_t *props_in, int64_t text_max, int64_t prec_words,
                                                     const int64_t *used, const int64_t *base, uint16_t *text_out,
                                                     uint32_t *props_out, int n_docs) {
    const int doc = blockIdx.x;
    if (doc >= n_docs) return;
    const int64_t tu = used[2 * doc], pu = used[2 * doc + 1], tb = base[2 * doc], pb = base[2 * doc + 1];
    const int64_t o0 = off[doc], n = off[doc + 1] - o0;
    const uint16_t *ts = text_in + o0 * text_max + doc;   // the generator's region (gen_begin)
    const uint32_t *ps = props_in + o0 * prec_words + doc;
    for (int64_t i = threadIdx.x; i < tu; i += blockDim.x) text_out[tb + i] = ts[i];
    for (int64_t i = threadIdx.x; i < pu; i += blockDim.x) props_out[pb + i] = ps[i];
    mt_op_rec *o = ops + o0;
    for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
        mt_op_rec op = o[k];
        if (op.kind == MT_OP_INSERT && !(op.flags & MT_F_MARKER)) op.payload += (uint32_t)tb;
        if (op.props != MT_NO_PROPS) op.props += (uint32_t)pb;
        o[k] = op;
    }
}

mt_batch *mt_generate(mt_handle *h, const mt_gen_cfg *cfg, uint32_t doc_index_base,
                      int32_t *view_len_trace) {
    return mt_generate_docs(h, cfg, doc_index_base, nullptr, nullptr, view_len_trace);
}

// mt_generate_docs' device work into batch b (sized by the caller, who frees it on failure and
// clears st.gen_off / st.gen_ids, which point at buffers of this function while it runs).
static int generate_into(mt_handle *h, mt_batch *b, mt_gen_cfg cfg, uint32_t doc_index_base, const int64_t *off,
                         bool own_lengths, const int32_t *doc_ids, int32_t *view_len_trace) {
    const int64_t N = h->n_docs;
    // every document's region at fixed strides per message (gen_begin)
    int64_t tstride = (int64_t)cfg.ops * cfg.text_max + 1;
    int64_t pstride = (int64_t)cfg.ops * (1 + 2 * (int64_t)cfg.max_keys_per_op) + 1;
    DevBuf<int32_t> d_fail, d_trace, d_ids;   // d_ids: the documents' global indices (their draws)
    DevBuf<int64_t> d_used;
    if (view_len_trace) HIPCHK(h, d_trace.alloc((size_t)b->n_ops * 4));
    HIPCHK(h, batch_alloc(b));
    HIPCHK(h, d_fail.alloc(N));
    HIPCHK(h, d_used.alloc(2 * N));
    HIPCHK(h, hipMemcpy(b->off, off, (N + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(d_fail.p, 0, N * 4));
    if (!set_order(b, off)) return MT_E_HIP;
    h->st.gen_off = own_lengths ? b->off : nullptr;   // (the generator kernels' lengths)
    if (doc_ids) {
        HIPCHK(h, d_ids.alloc(N));
        HIPCHK(h, hipMemcpy(d_ids.p, doc_ids, N * 4, hipMemcpyHostToDevice));
    }
    h->st.gen_ids = d_ids.p;
    HIPCHK(h, hipMemsetAsync(h->st.stats, 0, MT_STATS_WORDS * sizeof(uint32_t), h->stream));
    // k_generate / k_generate_paged: the same parameters but the last, the tier's capacities
    const int gw = 2 * (cfg.writers + 1);
    auto launch = [&](const Pick &p, void *caps) {
        void *a[] = {&h->st, &cfg, &doc_index_base, &b->ops, &b->text, &b->props, &tstride, &pstride, &d_fail.p,
                     &d_trace.p, &d_used.p, caps};
        return launch_variant(p, h->n_docs, h->stream, a);
    };
    if (h->lds.S > 0) {
        TierCaps caps = h->lds;
        HIPCHK(h, launch(pick_flat(K_GENERATE, facts(h), caps, gw), &caps));
    } else {
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->st.retry, 1, h->n_docs, h->stream));
    }
    if (h->st.PP > 0) {
        for (PagedCaps pc : {h->pg_tight, h->pg_full})
            if (pc.PP) HIPCHK(h, launch(pick_paged(K_GENERATE_PAGED, facts(h), pc, false, gw), &pc));
    } else {
        TierCaps caps = glb_caps(h);
        HIPCHK(h, launch(pick_flat(K_GENERATE, facts(h), caps, gw), &caps));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> f(N);
    HIPCHK(h, hipMemcpy(f.data(), d_fail.p, N * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < N; i++)
        if (f[i]) {
            DocHdr hd;
            hipMemcpy(&hd, h->st.hdr + i, sizeof(DocHdr), hipMemcpyDeviceToHost);
            h->err = "mt_generate: document " + std::to_string(i) + " failed with status " + std::to_string(f[i]) +
                     " (diagnostic " + std::to_string(hd.pad[HDR_DIAG]) + ")";
            return MT_E_INVALID;
        }
    // pack the per-document regions (u32 offsets address the whole batch)
    std::vector<int64_t> used((size_t)N * 2), base((size_t)N * 2);
    HIPCHK(h, hipMemcpy(used.data(), d_used.p, N * 16, hipMemcpyDeviceToHost));
    int64_t tt = 0, tp = 0;
    for (int64_t i = 0; i < N; i++) {
        base[2 * i] = tt;
        base[2 * i + 1] = tp;
        tt += used[2 * i];
        tp += used[2 * i + 1];
    }
    if (tt > (int64_t)UINT32_MAX || tp >= (int64_t)MT_NO_PROPS) {
        h->err = "mt_generate: the batch's text / property arenas exceed 32-bit offsets";
        return MT_E_INVALID;
    }
    DevBuf<uint16_t> nt;
    DevBuf<uint32_t> np;
    DevBuf<int64_t> d_base;
    HIPCHK(h, nt.alloc(tt));
    HIPCHK(h, np.alloc(tp));
    HIPCHK(h, d_base.alloc(2 * N));
    HIPCHK(h, hipMemcpy(d_base.p, base.data(), N * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gen_compact, dim3(h->n_docs), dim3(256), 0, h->stream, b->ops, b->off, b->text, b->props,
                       (int64_t)cfg.text_max, 1 + 2 * (int64_t)cfg.max_keys_per_op, d_used.p, d_base.p, nt.p, np.p,
                       h->n_docs);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipFree(b->text);
    hipFree(b->props);
    b->text = nt.release();
    b->props = np.release();
    b->text_len = tt;
    b->props_len = tp;
    if (view_len_trace) HIPCHK(h, hipMemcpy(view_len_trace, d_trace.p, b->n_ops * 16, hipMemcpyDeviceToHost));
    return 0;
}

mt_batch *mt_generate_docs(mt_handle *h, const mt_gen_cfg *cfg, uint32_t doc_index_base,
                           const int32_t *ops_per_doc, const int32_t *doc_ids, int32_t *view_len_trace) {
    if (!h || !cfg || cfg->writers < 1 || cfg->ops < 0) return nullptr;
    if (ops_per_doc)
        for (uint32_t d = 0; d < h->n_docs; d++)
            if (ops_per_doc[d] < 0) return nullptr;
    if (h->pending && mt_settle(h) != 0) return nullptr;
    h->max_cli = std::max(h->max_cli, cfg->writers);
    if (h->ordinals) {   // the generator's kernels keep no ordinals
        h->err = "mt_generate: not on a segment_ordinals handle";
        return nullptr;
    }
    if (hipSetDevice(h->device) != hipSuccess) return nullptr;
    auto *b = new mt_batch();
    b->device = h->device;
    b->n_docs = h->n_docs;
    const int64_t N = h->n_docs, ops = cfg->ops;
    std::vector<int64_t> off(N + 1);
    for (int64_t i = 0; i <= N; i++) off[i] = ops_per_doc ? (i ? off[i - 1] + ops_per_doc[i - 1] : 0) : i * ops;
    b->n_ops = off[N];
    b->text_len = off[N] * cfg->text_max + N;
    b->props_len = off[N] * (1 + 2 * (int64_t)cfg->max_keys_per_op) + N;
    const int rc = generate_into(h, b, *cfg, doc_index_base, off.data(), ops_per_doc != nullptr, doc_ids,
                                 view_len_trace);
    h->st.gen_off = nullptr;
    h->st.gen_ids = nullptr;
    if (rc) {
        if (h->err.empty()) h->err = "mt_generate failed";
        mt_batch_free(b);
        return nullptr;
    }
    return b;
}

int mt_generated_seeds(mt_handle *h, const mt_gen_cfg *cfg, uint32_t doc_index_base,
                       int64_t *seed_off, uint16_t *seed_text) {
    return mt_generated_seeds_docs(h, cfg, doc_index_base, nullptr, seed_off, seed_text);
}
int mt_generated_seeds_docs(mt_handle *h, const mt_gen_cfg *cfg, uint32_t doc_index_base, const int32_t *doc_ids,
                            int64_t *seed_off, uint16_t *seed_text) {
    if (!h || !cfg) return MT_E_INVALID;
    int64_t pos = 0;
    for (uint32_t doc = 0; doc < h->n_docs; doc++) {
        seed_off[doc] = pos;
        Rng r;
        rng_init(r, cfg->seed, doc_ids ? doc_ids[doc] : (int)(doc_index_base + doc));
        for (int i = 0; i < cfg->seed_len; i++) {
            (void)rng_next(r);
            const uint16_t ch = (uint16_t)(97 + rng_uniform(r, 26));
            if (seed_text) seed_text[pos] = ch;
            pos++;
        }
    }
    seed_off[h->n_docs] = pos;
    return 0;
}

int mt_batch_sizes(const mt_batch *b, uint64_t *n_ops, uint64_t *text_len, uint64_t *props_len) {
    if (!b) return MT_E_INVALID;
    if (n_ops) *n_ops = b->n_ops;
    if (text_len) *text_len = b->text_len;
    if (props_len) *props_len = b->props_len;
    return 0;
}

int mt_batch_download(const mt_batch *b, int64_t *doc_op_off, mt_op_rec *ops, uint16_t *text,
                      uint32_t *props) {
    if (!b) return MT_E_INVALID;
    if (hipSetDevice(b->device) != hipSuccess) return MT_E_HIP;
    if (doc_op_off && hipMemcpy(doc_op_off, b->off, (b->n_docs + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) return MT_E_HIP;
    if (ops && b->n_ops && hipMemcpy(ops, b->ops, b->n_ops * sizeof(mt_op_rec), hipMemcpyDeviceToHost) != hipSuccess) return MT_E_HIP;
    if (text && b->text_len && hipMemcpy(text, b->text, b->text_len * 2, hipMemcpyDeviceToHost) != hipSuccess) return MT_E_HIP;
    if (props && b->props_len && hipMemcpy(props, b->props, b->props_len * 4, hipMemcpyDeviceToHost) != hipSuccess) return MT_E_HIP;
    return 0;
}

// ---------------------------------------------------------------- read-out
struct HostDoc {
    DocHdr hdr;
    std::vector<int4> A;
    std::vector<u64> O;
    std::vector<uint4> B;
    std::vector<uint8_t> cnt;
    std::vector<uint16_t> text;
    std::vector<uint32_t> props;
    // paged documents: each row's page id, slot and directory position, and the page metadata
    std::vector<int32_t> rpage, rslot, rpos;
    std::vector<PageMeta> pmeta;
    int32_t oslot[2 * MT_OSLOTS];   // overlap slots {client, last seq}
    std::vector<uint16_t> ovf;      // paged: the overflow overlap arena (MT_OVF_BIT masks)
    // the B-tree's child counts by level (lv[0]: segments per leaf block, lv[depth - 1]: the
    // root's children), in order -- the shape the remote views' partial lengths follow
    std::vector<std::vector<int>> lv;
};
// document doc's paged arrays, host side (the growth step's slot mirror)
static PagedBase host_paged(const mt_handle *h, uint32_t doc) {
    const int s = h->bslot_h.empty() ? -1 : h->bslot_h[doc];
    return s >= 0 ? paged_base(h->st.big, (size_t)s) : paged_base(main_region(h->st), (size_t)doc);
}
static int fetch_doc(mt_handle *h, uint32_t doc, HostDoc &hd, bool with_text, bool with_props) {
    if (!h || doc >= h->n_docs) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    const DevState &st = h->st;
    HIPCHK(h, hipMemcpy(&hd.hdr, st.hdr + doc, sizeof(DocHdr), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(hd.oslot, st.oslot + (size_t)doc * 2 * MT_OSLOTS, sizeof(hd.oslot), hipMemcpyDeviceToHost));
    if (hd.hdr.pad[HDR_PAGED]) {
        // paged layout: concatenate the pages in directory order; leaf-block counts from
        // the page metadata
        const PagedBase pb = host_paged(h, doc);
        const size_t PP = pb.PP, slots = PP * MT_PG_SLOTS;
        const int np = hd.hdr.pad[HDR_NPAGES];
        std::vector<uint16_t> dir(std::max(np, 1));
        std::vector<PageMeta> meta(PP);
        std::vector<int4> pA(slots);
        std::vector<u64> pO(slots);
        std::vector<uint4> pB(slots);
        HIPCHK(h, hipMemcpy(dir.data(), pb.dir, np * sizeof(uint16_t), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(meta.data(), pb.meta, PP * sizeof(PageMeta), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(pA.data(), pb.A, slots * sizeof(int4), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(pO.data(), pb.O, slots * sizeof(u64), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(pB.data(), pb.B, slots * sizeof(uint4), hipMemcpyDeviceToHost));
        hd.ovf.assign(pb.ovf ? pb.OA : 0, 0);
        if (pb.ovf) HIPCHK(h, hipMemcpy(hd.ovf.data(), pb.ovf, (size_t)pb.OA * 2, hipMemcpyDeviceToHost));
        hd.A.clear();
        hd.O.clear();
        hd.B.clear();
        hd.cnt.clear();
        hd.rpage.clear();
        hd.rslot.clear();
        hd.rpos.clear();
        for (int q = 0; q < np; q++) {
            const PageMeta &m = meta[dir[q]];
            const size_t b0 = (size_t)dir[q] * MT_PG_SLOTS;
            for (int i = 0; i < m.nseg; i++) {
                hd.A.push_back(pA[b0 + i]);
                hd.O.push_back(pO[b0 + i]);
                hd.B.push_back(pB[b0 + i]);
                hd.rpage.push_back(dir[q]);
                hd.rslot.push_back(i);
                hd.rpos.push_back(q);
            }
            for (int k = 0; k < m.nblk; k++) hd.cnt.push_back((uint8_t)pm_bcnt(m, k));
        }
        {   // the levels: leaf blocks from the pages, level 1 = the pages in directory order,
            // levels >= 2 from the upper count arrays
            const int D = std::max(hd.hdr.depth, 1);
            hd.lv.assign(D, {});
            hd.lv[0].assign(hd.cnt.begin(), hd.cnt.end());
            if (D >= 2)
                for (int q = 0; q < np; q++) hd.lv[1].push_back(meta[dir[q]].nblk);
            if (D >= 3) {
                std::vector<uint8_t> cn((size_t)MT_LV * PP);
                HIPCHK(h, hipMemcpy(cn.data(), pb.cnt, cn.size(), hipMemcpyDeviceToHost));
                for (int l = 2; l < D; l++)
                    for (int b = 0; b < hd.hdr.n_blk[l]; b++) hd.lv[l].push_back(cn[(size_t)l * PP + b]);
            }
        }
        hd.pmeta = std::move(meta);
        hd.hdr.n_seg = (int)hd.A.size();
        hd.hdr.n_blk[0] = (int)hd.cnt.size();
        hd.A.resize(std::max<size_t>(hd.A.size(), 1));
        hd.O.resize(std::max<size_t>(hd.O.size(), 1));
        hd.B.resize(std::max<size_t>(hd.B.size(), 1));
        hd.cnt.resize(std::max<size_t>(hd.cnt.size(), 1));
    } else {
    const int n = hd.hdr.n_seg;
    hd.A.resize(std::max(n, 1));
    hd.O.resize(std::max(n, 1));
    hd.B.resize(std::max(n, 1));
    if (n) {
        HIPCHK(h, hipMemcpy(hd.A.data(), st.segA + (size_t)doc * st.S, n * sizeof(int4), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(hd.O.data(), st.segO + (size_t)doc * st.S, n * sizeof(u64), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(hd.B.data(), st.segB + (size_t)doc * st.S, n * sizeof(uint4), hipMemcpyDeviceToHost));
    }
    hd.cnt.resize((size_t)MT_LV * st.B);
    HIPCHK(h, hipMemcpy(hd.cnt.data(), st.cnt + (size_t)doc * MT_LV * st.B, MT_LV * st.B, hipMemcpyDeviceToHost));
    const int D = std::max(hd.hdr.depth, 1);
    hd.lv.assign(D, {});
    for (int l = 0; l < D; l++)
        for (int b = 0; b < hd.hdr.n_blk[l]; b++) hd.lv[l].push_back(hd.cnt[(size_t)l * st.B + b]);
    }
    const PagedBase ar = host_paged(h, doc);   // (the arenas of the document's region)
    if (with_text) {
        hd.text.resize(ar.T);
        HIPCHK(h, hipMemcpy(hd.text.data(), ar.text + (size_t)hd.hdr.text_half * ar.T, (size_t)ar.T * 2,
                            hipMemcpyDeviceToHost));
    }
    if (with_props) {
        const size_t words = (size_t)ar.P * MT_PREC;
        hd.props.resize(words);
        HIPCHK(h, hipMemcpy(hd.props.data(), ar.props + (size_t)hd.hdr.props_half * words, words * 4,
                            hipMemcpyDeviceToHost));
    }
    return 0;
}

int mt_get_status(mt_handle *h, int32_t *out_status) {
    if (!h || !out_status) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    std::vector<DocHdr> hs(h->n_docs);
    HIPCHK(h, hipMemcpy(hs.data(), h->st.hdr, h->n_docs * sizeof(DocHdr), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < h->n_docs; i++) out_status[i] = hs[i].status;
    return 0;
}

int mt_get_length(mt_handle *h, uint32_t doc, uint32_t *out) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, false);
    if (rc) return rc;
    uint32_t len = 0;
    for (int i = 0; i < hd.hdr.n_seg; i++)
        if (hd.A[i].z == MT_RSEQ_NONE) len += hd.A[i].x;
    *out = len;
    return 0;
}

int mt_get_text(mt_handle *h, uint32_t doc, uint16_t *out, uint32_t cap, uint32_t *out_len) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, true, false);
    if (rc) return rc;
    uint32_t n = 0;
    for (int i = 0; i < hd.hdr.n_seg; i++) {
        const int4 a = hd.A[i];
        const uint4 b = hd.B[i];
        if (a.z != MT_RSEQ_NONE || (b.z & MT_MARKER_BIT)) continue;
        for (int j = 0; j < a.x; j++) {
            if (out && n < cap) out[n] = hd.text[b.x + j];
            n++;
        }
    }
    if (out_len) *out_len = n;
    return 0;
}

// mt_get_texts / mt_get_texts_device: the counting pass, the prefix sums, the gather.
static int get_texts(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start, const int32_t *end,
                     uint16_t marker_unit, int64_t *off, uint16_t *out, void *out_dev, uint64_t cap, bool device) {
    if (!h || !off) return MT_E_INVALID;
    int rc = check_queries(h, "mt_get_texts", n, docs);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    ReadTimer &tm = h->tm_txt;
    tm.timed = 0;
    if (n == 0) return empty_offsets(h, {off}, device);
    QueryCols qc;   // extra: len[n], off[n + 1]
    HIPCHK(h, qc.upload(n, {docs, start, end}, ((size_t)n * 2 + 1) * 8));
    const uint32_t *d_docs = (const uint32_t *)qc.col[0];
    const int32_t *d_start = (const int32_t *)qc.col[1], *d_end = (const int32_t *)qc.col[2];
    int64_t *d_len = (int64_t *)qc.extra, *d_off = device ? off : d_len + n;
    HIPCHK(h, tm.begin(0, h->stream));
    hipLaunchKernelGGL(k_text_count, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start, d_end,
                       (int)marker_unit, d_len);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(0, h->stream));
    int64_t total = 0;
    if ((rc = scan_counts(h, n, 1, &d_len, &off, device, &total))) return rc;
    tm.timed = 1;
    rc = after_counts(h, device ? !out_dev : !out, cap >= (uint64_t)total, total == 0, [&] {
        return "mt_get_texts: the output holds " + std::to_string(cap) + " units, the results need " +
               std::to_string(total);
    });
    if (rc != RO_GATHER) return rc;
    if (!device) HIPCHK(h, hipMemcpy(d_off, off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    OutStage<uint16_t> text;
    HIPCHK(h, text.open(out_dev, device, (size_t)total));
    // MT_TEXT_PER_SEGMENT=1: the per-segment copy (the A/B of tools/readout_probe.py)
    const char *ps = getenv("MT_TEXT_PER_SEGMENT");
    const bool per_seg = ps && ps[0] == '1';
    HIPCHK(h, tm.begin(1, h->stream));
    if (per_seg)
        hipLaunchKernelGGL(k_text_gather<true>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start,
                           d_end, (int)marker_unit, d_off, text.p);
    else
        hipLaunchKernelGGL(k_text_gather<false>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start,
                           d_end, (int)marker_unit, d_off, text.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    tm.timed = 2;
    HIPCHK(h, text.copy_out(out, (size_t)total));
    return 0;
}

int mt_get_texts(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start, const int32_t *end,
                 uint16_t marker_unit, int64_t *off, uint16_t *out, uint64_t cap) {
    return get_texts(h, n, docs, start, end, marker_unit, off, out, nullptr, cap, false);
}

int mt_get_texts_device(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start, const int32_t *end,
                        uint16_t marker_unit, void *off_dev, void *out_dev, uint64_t cap) {
    return get_texts(h, n, docs, start, end, marker_unit, (int64_t *)off_dev, nullptr, out_dev, cap, true);
}

int mt_last_text_ms(mt_handle *h, float *out) {
    if (!h || !out) return MT_E_INVALID;
    return read_timer(h, h->tm_txt, out);
}

// mt_get_prop_runs_bulk / mt_get_prop_runs_bulk_device: get_texts' shape with two counts per
// query (runs, record words), so two prefix sums and two outputs.
static int get_prop_runs_bulk(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start,
                              const int32_t *end, int64_t *run_off, int64_t *word_off, void *runs, uint64_t cap_runs,
                              void *records, uint64_t cap_words, bool device) {
    if (!h || !run_off || !word_off) return MT_E_INVALID;
    int rc = check_queries(h, "mt_get_prop_runs_bulk", n, docs);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    ReadTimer &tm = h->tm_prp;
    tm.timed = 0;
    if (n == 0) return empty_offsets(h, {run_off, word_off}, device);
    QueryCols qc;   // extra: the run and word counts [n] each, the two offset arrays [n + 1] each
    HIPCHK(h, qc.upload(n, {docs, start, end}, ((size_t)n * 4 + 2) * 8));
    const uint32_t *d_docs = (const uint32_t *)qc.col[0];
    const int32_t *d_start = (const int32_t *)qc.col[1], *d_end = (const int32_t *)qc.col[2];
    int64_t *d_cnt[2] = {(int64_t *)qc.extra, (int64_t *)qc.extra + n};   // runs, words
    int64_t *off[2] = {run_off, word_off};
    int64_t *d_roff = device ? run_off : d_cnt[1] + n, *d_woff = device ? word_off : d_roff + n + 1;
    HIPCHK(h, tm.begin(0, h->stream));
    hipLaunchKernelGGL(k_props_count, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start, d_end,
                       d_cnt[0], d_cnt[1]);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(0, h->stream));
    int64_t total[2] = {0, 0};
    if ((rc = scan_counts(h, n, 2, d_cnt, off, device, total))) return rc;
    tm.timed = 1;
    if (!records) cap_words = 0;
    rc = after_counts(h, !runs, cap_runs >= (uint64_t)total[0] && cap_words >= (uint64_t)total[1], total[0] == 0, [&] {
        return "mt_get_prop_runs_bulk: the outputs hold " + std::to_string(cap_runs) + " runs and " +
               std::to_string(cap_words) + " words, the results need " + std::to_string(total[0]) + " runs and " +
               std::to_string(total[1]) + " words";
    });
    if (rc != RO_GATHER) return rc;
    if (!device) {
        HIPCHK(h, hipMemcpy(d_roff, run_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d_woff, word_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    }
    OutStage<uint32_t> g_runs, g_recs;   // a run is three words
    HIPCHK(h, g_runs.open(runs, device, (size_t)total[0] * 3));
    HIPCHK(h, g_recs.open(records, device, (size_t)total[1]));
    HIPCHK(h, tm.begin(1, h->stream));
    hipLaunchKernelGGL(k_props_gather, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start, d_end,
                       d_roff, d_woff, g_runs.p, g_recs.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    tm.timed = 2;
    HIPCHK(h, g_runs.copy_out(runs, (size_t)total[0] * 3));
    HIPCHK(h, g_recs.copy_out(records, (size_t)total[1]));
    return 0;
}

int mt_get_prop_runs_bulk(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start, const int32_t *end,
                          int64_t *run_off, int64_t *word_off, uint32_t *runs, uint64_t cap_runs, uint32_t *records,
                          uint64_t cap_words) {
    return get_prop_runs_bulk(h, n, docs, start, end, run_off, word_off, runs, cap_runs, records, cap_words, false);
}

int mt_get_prop_runs_bulk_device(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start,
                                 const int32_t *end, void *run_off_dev, void *word_off_dev, void *runs_dev,
                                 uint64_t cap_runs, void *records_dev, uint64_t cap_words) {
    return get_prop_runs_bulk(h, n, docs, start, end, (int64_t *)run_off_dev, (int64_t *)word_off_dev, runs_dev,
                              cap_runs, records_dev, cap_words, true);
}

int mt_last_props_ms(mt_handle *h, float *out) {
    if (!h || !out) return MT_E_INVALID;
    return read_timer(h, h->tm_prp, out);
}

// mt_walk_segments / mt_walk_segments_device: get_prop_runs_bulk's shape with three counts per
// query (rows, text units, record words), so three prefix sums and three outputs; the count
// pass also leaves every query's end as the leaf action sees it for the gather.
// mt_walk_segments_view*: the same in a (refSeq, client) view per query.  The count pass marks the
// queries of views with N != L; their visit lists and counts are computed here (walk_on_host,
// below host_search) and patched into the counts before the prefix sums, the gather skips them
// and their rows, texts and records are written into their slots after it.
struct HostWalk {   // a query answered on the host
    uint32_t q;
    std::vector<mt_walk_row> rows;
    std::vector<uint16_t> text;
    std::vector<uint32_t> recs;
};
static int walk_on_host(mt_handle *h, std::vector<uint32_t> todo, const uint32_t *docs, const int32_t *start,
                        const int32_t *end, const int32_t *ref_seq, const int32_t *client, uint32_t what,
                        std::vector<HostWalk> &out);
static int walk_segments(mt_handle *h, const char *name, uint32_t n, const uint32_t *docs, const int32_t *start,
                         const int32_t *end, const int32_t *ref_seq, const int32_t *client, uint32_t what,
                         int64_t *row_off, int64_t *text_off, int64_t *word_off, void *rows, uint64_t cap_rows,
                         void *text, uint64_t cap_text, void *records, uint64_t cap_words, bool device) {
    if (!h || !row_off || !text_off || !word_off) return MT_E_INVALID;
    if ((ref_seq == nullptr) != (client == nullptr)) {
        h->err = std::string(name) + ": ref_seq and client are both NULL or both given";
        return MT_E_INVALID;
    }
    if (what & ~(MT_WALK_TEXT | MT_WALK_PROPS)) {
        h->err = std::string(name) + ": undefined bits in what (" + std::to_string(what) + ")";
        return MT_E_INVALID;
    }
    int rc = check_queries(h, name, n, docs);
    if (rc) return rc;
    for (uint32_t q = 0; start && q < n; q++)
        if (start[q] < 0) {
            h->err = std::string(name) + ": query " + std::to_string(q) + ": start below 0";
            return MT_E_INVALID;
        }
    bool view = false;   // some query asks for a view other than the replica's own
    for (uint32_t q = 0; client && q < n; q++) {
        if (client[q] < 0) {
            h->err = std::string(name) + ": query " + std::to_string(q) + ": negative client";
            return MT_E_INVALID;
        }
        view = view || client[q] != 0;
    }
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    ReadTimer &tm = h->tm_walk;
    tm.timed = 0;
    h->wv_n = n;
    h->wv_host = h->wv_skip = 0;
    if (n == 0) return empty_offsets(h, {row_off, text_off, word_off}, device);
    // extra: the three counts [n] each, the three offset arrays [n + 1] each, the ends [n]; in a
    // view the refSeqs, the clients and the marks [n] each
    const size_t cnt_w = (size_t)n * 3, off_w = ((size_t)n + 1) * 3, end_b = ((size_t)n * 4 + 7) & ~(size_t)7;
    QueryCols qc;
    HIPCHK(h, qc.upload(n, {docs, start, end}, (cnt_w + off_w) * 8 + end_b * (view ? 7 : 1)));
    const uint32_t *d_docs = (const uint32_t *)qc.col[0];
    const int32_t *d_start = (const int32_t *)qc.col[1], *d_end = (const int32_t *)qc.col[2];
    int64_t *base = (int64_t *)qc.extra;
    int64_t *d_cnt[3] = {base, base + n, base + 2 * (size_t)n};   // rows, units, words
    int64_t *off[3] = {row_off, text_off, word_off};
    int64_t *d_off[3];
    for (int i = 0; i < 3; i++) d_off[i] = device ? off[i] : base + cnt_w + (size_t)i * (n + 1);
    int32_t *d_ends = (int32_t *)(base + cnt_w + off_w);
    WalkViewArgs<false> no_view;
    WalkViewArgs<true> va{nullptr, nullptr, nullptr, nullptr, 0};
    // the page ids the count pass's LDS array holds: the handle's page capacities, 32 KB at the most
    const int lds_pages = view ? std::min(std::max({(int)h->st.PP, (int)h->st.big.PP, 1}), 8192) : 0;
    if (view) {
        uint8_t *vb = (uint8_t *)d_ends + end_b;
        HIPCHK(h, hipMemcpy(vb, ref_seq, (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(vb + end_b, client, (size_t)n * 4, hipMemcpyHostToDevice));
        va = WalkViewArgs<true>{(const int32_t *)vb, (const int32_t *)(vb + end_b), (int32_t *)(vb + 2 * end_b),
                                (int32_t *)(vb + 3 * end_b), lds_pages};
    }
    // MT_LOCATE_ROW_WALK=1: walk from row 0 (the A/B of tools/walk_probe.py)
    const char *rw = getenv("MT_LOCATE_ROW_WALK");
    const int skip = !(rw && rw[0] == '1');
    HIPCHK(h, tm.begin(0, h->stream));
    if (view)
        hipLaunchKernelGGL(k_walk_count<true>, dim3(n), dim3(MT_WAVE), (size_t)lds_pages * 4, h->stream, h->st, (int)n, d_docs, d_start,
                           d_end, what, skip, d_cnt[0], d_cnt[1], d_cnt[2], d_ends, va);
    else
        hipLaunchKernelGGL(k_walk_count<false>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start,
                           d_end, what, skip, d_cnt[0], d_cnt[1], d_cnt[2], d_ends, no_view);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(0, h->stream));
    std::vector<HostWalk> hw;
    if (view) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<int32_t> mark(n);
        HIPCHK(h, hipMemcpy(mark.data(), va.mark, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> todo;
        for (uint32_t q = 0; q < n; q++) {
            if (mark[q] == MT_WALKQ_INVALID) {
                h->err = std::string(name) + ": query " + std::to_string(q) + ": remote view of document " +
                         std::to_string(docs ? docs[q] : q) + " with refSeq " + std::to_string(ref_seq[q]) +
                         " outside the collab window [minSeq, currentSeq]";
                return MT_E_INVALID;
            }
            if (mark[q] == MT_WALKQ_HOST) todo.push_back(q);
            h->wv_skip += mark[q] == MT_WALKQ_SKIP;
        }
        if ((rc = walk_on_host(h, todo, docs, start, end, ref_seq, client, what, hw))) return rc;
        if (!hw.empty()) {   // the three count arrays are adjacent: one copy each way
            std::vector<int64_t> cnt(cnt_w);
            HIPCHK(h, hipMemcpy(cnt.data(), base, cnt_w * 8, hipMemcpyDeviceToHost));
            for (const HostWalk &w : hw) {
                cnt[w.q] = (int64_t)w.rows.size();
                cnt[(size_t)n + w.q] = (int64_t)w.text.size();
                cnt[2 * (size_t)n + w.q] = (int64_t)w.recs.size();
            }
            HIPCHK(h, hipMemcpy(base, cnt.data(), cnt_w * 8, hipMemcpyHostToDevice));
        }
        h->wv_host = (int64_t)hw.size();
    }
    int64_t total[3] = {0, 0, 0};
    if ((rc = scan_counts(h, n, 3, d_cnt, off, device, total))) return rc;
    tm.timed = 1;
    if (!text) cap_text = 0;
    if (!records) cap_words = 0;
    const bool fits = cap_rows >= (uint64_t)total[0] && cap_text >= (uint64_t)total[1] && cap_words >= (uint64_t)total[2];
    rc = after_counts(h, !rows, fits, total[0] == 0, [&] {
        return std::string(name) + ": the outputs hold " + std::to_string(cap_rows) + " rows, " +
               std::to_string(cap_text) + " text units and " + std::to_string(cap_words) + " words, the results need " +
               std::to_string(total[0]) + " rows, " + std::to_string(total[1]) + " text units and " +
               std::to_string(total[2]) + " words";
    });
    if (rc != RO_GATHER) return rc;
    if (!device)
        for (int i = 0; i < 3; i++)
            HIPCHK(h, hipMemcpy(d_off[i], off[i], ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    OutStage<mt_walk_row> g_rows;
    OutStage<uint16_t> g_text;
    OutStage<uint32_t> g_recs;
    HIPCHK(h, g_rows.open(rows, device, (size_t)total[0]));
    HIPCHK(h, g_text.open(text, device, (size_t)total[1]));
    HIPCHK(h, g_recs.open(records, device, (size_t)total[2]));
    HIPCHK(h, tm.begin(1, h->stream));
    if (view)
        hipLaunchKernelGGL(k_walk_gather<true>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start,
                           d_end, what, skip, (const int32_t *)d_ends, (const int64_t *)d_off[0],
                           (const int64_t *)d_off[1], (const int64_t *)d_off[2], g_rows.p, g_text.p, g_recs.p, va);
    else
        hipLaunchKernelGGL(k_walk_gather<false>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_start,
                           d_end, what, skip, (const int32_t *)d_ends, (const int64_t *)d_off[0],
                           (const int64_t *)d_off[1], (const int64_t *)d_off[2], g_rows.p, g_text.p, g_recs.p, no_view);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    tm.timed = 2;
    // the host-answered queries' slots (the offsets' totals hold their counts, so the capacities
    // were checked with them): into the staged outputs, which copy_out then hands over
    std::vector<int64_t> offs_dev;   // (the _device form: the offsets are in device memory)
    if (device && !hw.empty()) {
        offs_dev.resize(3 * ((size_t)n + 1));
        for (int i = 0; i < 3; i++)
            HIPCHK(h, hipMemcpy(offs_dev.data() + (size_t)i * (n + 1), off[i], ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    }
    for (const HostWalk &w : hw) {
        int64_t o3[3];
        for (int i = 0; i < 3; i++) o3[i] = device ? offs_dev[(size_t)i * (n + 1) + w.q] : off[i][w.q];
        if (!w.rows.empty())
            HIPCHK(h, hipMemcpy(g_rows.p + o3[0], w.rows.data(), w.rows.size() * sizeof(mt_walk_row), hipMemcpyHostToDevice));
        if (!w.text.empty()) HIPCHK(h, hipMemcpy(g_text.p + o3[1], w.text.data(), w.text.size() * 2, hipMemcpyHostToDevice));
        if (!w.recs.empty()) HIPCHK(h, hipMemcpy(g_recs.p + o3[2], w.recs.data(), w.recs.size() * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(h, g_rows.copy_out(rows, (size_t)total[0]));
    HIPCHK(h, g_text.copy_out(text, (size_t)total[1]));
    HIPCHK(h, g_recs.copy_out(records, (size_t)total[2]));
    return 0;
}

int mt_walk_segments(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start, const int32_t *end,
                     uint32_t what, int64_t *row_off, int64_t *text_off, int64_t *word_off, mt_walk_row *rows,
                     uint64_t cap_rows, uint16_t *text, uint64_t cap_text, uint32_t *records, uint64_t cap_words) {
    return walk_segments(h, "mt_walk_segments", n, docs, start, end, nullptr, nullptr, what, row_off, text_off, word_off,
                         rows, cap_rows, text, cap_text, records, cap_words, false);
}

int mt_walk_segments_device(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start, const int32_t *end,
                            uint32_t what, void *row_off_dev, void *text_off_dev, void *word_off_dev, void *rows_dev,
                            uint64_t cap_rows, void *text_dev, uint64_t cap_text, void *records_dev,
                            uint64_t cap_words) {
    return walk_segments(h, "mt_walk_segments", n, docs, start, end, nullptr, nullptr, what, (int64_t *)row_off_dev,
                         (int64_t *)text_off_dev, (int64_t *)word_off_dev, rows_dev, cap_rows, text_dev, cap_text,
                         records_dev, cap_words, true);
}

int mt_walk_segments_view(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start, const int32_t *end,
                          const int32_t *ref_seq, const int32_t *client, uint32_t what, int64_t *row_off,
                          int64_t *text_off, int64_t *word_off, mt_walk_row *rows, uint64_t cap_rows, uint16_t *text,
                          uint64_t cap_text, uint32_t *records, uint64_t cap_words) {
    return walk_segments(h, "mt_walk_segments_view", n, docs, start, end, ref_seq, client, what, row_off, text_off,
                         word_off, rows, cap_rows, text, cap_text, records, cap_words, false);
}

int mt_walk_segments_view_device(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *start,
                                 const int32_t *end, const int32_t *ref_seq, const int32_t *client, uint32_t what,
                                 void *row_off_dev, void *text_off_dev, void *word_off_dev, void *rows_dev,
                                 uint64_t cap_rows, void *text_dev, uint64_t cap_text, void *records_dev,
                                 uint64_t cap_words) {
    return walk_segments(h, "mt_walk_segments_view", n, docs, start, end, ref_seq, client, what, (int64_t *)row_off_dev,
                         (int64_t *)text_off_dev, (int64_t *)word_off_dev, rows_dev, cap_rows, text_dev, cap_text,
                         records_dev, cap_words, true);
}

int mt_last_walk_view(mt_handle *h, int64_t *out, float *ms) {
    if (!h || !out) return MT_E_INVALID;
    out[0] = h->wv_n;
    out[1] = h->wv_host;
    out[2] = h->wv_skip;
    if (ms) return read_timer(h, h->tm_walk, ms);
    return 0;
}

int mt_last_walk_ms(mt_handle *h, float *out) {
    if (!h || !out) return MT_E_INVALID;
    return read_timer(h, h->tm_walk, out);
}

int mt_get_prop_runs(mt_handle *h, uint32_t doc, uint32_t *runs, uint32_t cap_runs,
                     uint32_t *n_runs, uint32_t *records, uint32_t cap_words, uint32_t *n_words) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, true);
    if (rc) return rc;
    uint32_t nr = 0, nw = 0, pos = 0;
    uint32_t cur_h = 0xFFFFFFFFu, cur_start = 0, cur_len = 0, cur_rec = 0;
    auto same = [&](uint32_t a, uint32_t b) {
        if (a == 0 || b == 0) return a == b;
        const uint32_t *x = &hd.props[(size_t)a * MT_PREC], *y = &hd.props[(size_t)b * MT_PREC];
        if (x[0] != y[0]) return false;
        for (uint32_t i = 0; i < 2 * x[0]; i++)
            if (x[1 + i] != y[1 + i]) return false;
        return true;
    };
    auto flush = [&]() {
        if (cur_h == 0xFFFFFFFFu) return;
        if (runs && nr < cap_runs) {
            runs[3 * nr] = cur_start;
            runs[3 * nr + 1] = cur_len;
            runs[3 * nr + 2] = cur_rec;
        }
        nr++;
    };
    for (int i = 0; i < hd.hdr.n_seg; i++) {
        const int4 a = hd.A[i];
        if (a.z != MT_RSEQ_NONE) continue;
        const uint32_t ph = hd.B[i].y;
        if (cur_h != 0xFFFFFFFFu && same(cur_h, ph)) {
            cur_len += a.x;
        } else {
            flush();
            cur_h = ph;
            cur_start = pos;
            cur_len = a.x;
            if (ph == 0) {
                cur_rec = 0xFFFFFFFFu;
            } else {
                cur_rec = nw;
                const uint32_t *x = &hd.props[(size_t)ph * MT_PREC];
                for (uint32_t k = 0; k < 1 + 2 * x[0]; k++) {
                    if (records && nw < cap_words) records[nw] = x[k];
                    nw++;
                }
            }
        }
        pos += a.x;
    }
    flush();
    if (n_runs) *n_runs = nr;
    if (n_words) *n_words = nw;
    return 0;
}

int mt_get_segments(mt_handle *h, uint32_t doc, int32_t *rows, uint32_t cap_rows,
                    uint32_t *n_rows, int32_t *leaves, uint32_t cap_leaves, uint32_t *n_leaves) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, false);
    if (rc) return rc;
    const int n = hd.hdr.n_seg;
    for (int i = 0; i < n && rows && (uint32_t)i < cap_rows; i++) {
        const int4 a = hd.A[i];
        const uint4 b = hd.B[i];
        int32_t *r = rows + 8 * i;
        // live documents: an unacked insert / local remove reads UnassignedSequenceNumber (-1)
        const bool lins = a.y >= MT_LOCAL_BASE, lrem = a.z >= MT_LOCAL_BASE;
        r[0] = a.x;
        r[1] = lins ? -1 : a.y;
        r[2] = (int)(short)(a.w & 0xFFFF);
        r[3] = lrem ? -1 : a.z;
        r[4] = a.z == MT_RSEQ_NONE ? MT_RSEQ_NONE : (int)(short)((uint32_t)a.w >> 16);
        {   // removedClientOverlap's length: the slot bits, or an overflow set's count
            const u64 o = hd.O[i];
            const size_t off = (uint32_t)o;
            r[5] = !(o & MT_OVF_BIT) ? __builtin_popcountll(o) : (off < hd.ovf.size() ? (int)hd.ovf[off] : -1);
        }
        r[6] = (b.z & MT_MARKER_BIT) ? (int32_t)b.x : -1;
        r[7] = b.y ? 1 : 0;
    }
    if (n_rows) *n_rows = (uint32_t)n;
    const int nb0 = hd.hdr.n_blk[0];
    for (int b = 0; b < nb0 && leaves && (uint32_t)b < cap_leaves; b++) leaves[b] = hd.cnt[b];
    if (n_leaves) *n_leaves = (uint32_t)nb0;
    return 0;
}

// ---------------------------------------------------------------- segment read-outs
// Views of one fetched document for mt_get_containing_segment / mt_get_segment_by_uid /
// mt_get_view_lengths (the device's view_len, MT/mergeTree.ts:1692-1732; client 0 = this
// replica: its local net length whatever the refSeq).
struct HostView {
    int r, c, cs;   // refSeq, short client, c's overlap slot (0: none)
    bool local;
};
static int host_view_setup(mt_handle *h, uint32_t doc, const HostDoc &hd, int32_t ref_seq, int32_t client,
                           HostView &v) {
    (void)doc;
    v.r = ref_seq;
    v.c = client;
    v.cs = 0;
    v.local = client == 0;
    if (v.local) return 0;
    if (ref_seq < hd.hdr.min_seq || ref_seq > hd.hdr.cur_seq) {
        h->err = "remote view: refSeq outside the collab window [minSeq, currentSeq]";
        return MT_E_INVALID;
    }
    for (int i = 0; i < MT_OSLOTS; i++)
        if (hd.oslot[2 * i] == client) {
            v.cs = i + 1;
            break;
        }
    return 0;
}
// row i in view v: {inserted in the view, removed in the view} (nodeLength's two tests)
static void host_view_vis(const HostDoc &hd, const HostView &v, int i, bool &ins, bool &gone) {
    const int4 a = hd.A[i];
    const int cli = (int)(short)(a.w & 0xFFFF), rcli = (int)(short)((uint32_t)a.w >> 16);
    const u64 o = hd.O[i];
    bool ovl = v.cs >= 1 && ((o >> (v.cs - 1)) & 1ull);
    if (o & MT_OVF_BIT) {   // an overflow set: the segment's whole overlap list
        ovl = false;
        const size_t off = (uint32_t)o;
        const size_t n = off < hd.ovf.size() ? hd.ovf[off] : 0;
        for (size_t k = 1; k <= n && off + k < hd.ovf.size(); k++) ovl = ovl || hd.ovf[off + k] == (uint16_t)v.c;
    }
    ins = cli == v.c || (a.y != -1 && a.y <= v.r);
    gone = a.z != MT_RSEQ_NONE && (rcli == v.c || ovl || (a.z != -1 && a.z <= v.r));
}
// a leaf's nodeLength in the view
static int host_view_len(const HostDoc &hd, const HostView &v, int i) {
    const int4 a = hd.A[i];
    if (v.local) return a.z == MT_RSEQ_NONE ? a.x : 0;
    bool ins, gone;
    host_view_vis(hd, v, i, ins, gone);
    return ins && !gone ? a.x : 0;
}
// The leaf's term in its ancestors' PartialSequenceLengths (MT/partialLengths.ts): +len at its
// insert, -len at its removal, each counted when the view holds it (getBranchPartialLength
// :455-486 adds every entry at or below refSeq and the client's own later ones, overlap
// removes included via clientSeqNumbers :581-590).  The two are independent: a view below the
// client's latest refSeq can see a segment removed (by the client) but not inserted, and then
// the segment counts -len -- the reference's interior node lengths there differ from the sum
// of their leaves' nodeLength (oracle/mt_oracle.c seg_partial; pinned on every view of
// tests/golden/ref_readouts*).  In any other view it equals the leaf's nodeLength.
static int host_seg_partial(const HostDoc &hd, const HostView &v, int i) {
    const int4 a = hd.A[i];
    if (v.local) return a.z == MT_RSEQ_NONE ? a.x : 0;   // blockLength: cachedLength
    bool ins, gone;
    host_view_vis(hd, v, i, ins, gone);
    return a.x * ((int)ins - (int)gone);
}
// The tree's node lengths in view v: P[l][b] = node b of level l's length (partial lengths),
// first[l][b] = its first child (a segment row at level 0, a node of level l - 1 above).
struct HostTree {
    std::vector<std::vector<int>> P, first;
};
static void host_tree(const HostDoc &hd, const HostView &v, HostTree &t) {
    const int D = (int)hd.lv.size();
    t.P.assign(D, {});
    t.first.assign(D, {});
    for (int l = 0; l < D; l++) {
        int f = 0;
        for (int b = 0; b < (int)hd.lv[l].size(); b++) {
            t.first[l].push_back(f);
            int sum = 0;
            for (int k = f; k < f + hd.lv[l][b]; k++)
                sum += l == 0 ? (k < hd.hdr.n_seg ? host_seg_partial(hd, v, k) : 0)
                              : (k < (int)t.P[l - 1].size() ? t.P[l - 1][k] : 0);
            t.P[l].push_back(sum);
            f += hd.lv[l][b];
        }
    }
}
// MergeTree.getPosition(node, refSeq, clientId) (:1619-1636) of row i: the nodeLength of its
// earlier siblings and of each ancestor's earlier siblings (interior ones: partial lengths)
static int host_position(const HostDoc &hd, const HostView &v, const HostTree &t, int i) {
    const int D = (int)hd.lv.size();
    int x = i, p = 0;
    for (int l = 0; l < D; l++) {
        int b = 0;   // x's parent at level l
        while (b + 1 < (int)t.first[l].size() && t.first[l][b + 1] <= x) b++;
        for (int k = t.first[l].empty() ? x : t.first[l][b]; k < x; k++)
            p += l == 0 ? host_view_len(hd, v, k) : t.P[l - 1][k];
        x = b;
    }
    return p;
}
// the fields of row i (and, on a segment_ordinals handle, its ordinal from the per-node
// characters: ancestors below the root, then its own)
static int host_seg_info(mt_handle *h, uint32_t doc, const HostDoc &hd, int i, mt_seg_info *out, uint16_t *text,
                         uint32_t text_cap) {
    const int4 a = hd.A[i];
    const uint4 b = hd.B[i];
    const bool lins = a.y >= MT_LOCAL_BASE, lrem = a.z >= MT_LOCAL_BASE && a.z != MT_RSEQ_NONE;
    out->row = i;
    out->uid = b.z & ~MT_MARKER_BIT;
    out->length = a.x;
    out->seq = lins ? -1 : a.y;
    out->client = (int)(short)(a.w & 0xFFFF);
    out->removed_seq = lrem ? -1 : a.z;
    out->removed_client = a.z == MT_RSEQ_NONE ? MT_RSEQ_NONE : (int)(short)((uint32_t)a.w >> 16);
    const bool marker = (b.z & MT_MARKER_BIT) != 0;
    out->marker_ref_type = marker ? (int32_t)b.x : -1;
    out->text_len = 0;
    if (!marker && text) {
        for (int j = 0; j < a.x && (uint32_t)j < text_cap; j++) text[j] = hd.text[b.x + j];
        out->text_len = std::min<int>(a.x, (int)text_cap);
    }
    out->ordinal_len = -1;
    if (h->ordinals && !hd.hdr.pad[HDR_PAGED]) {
        const size_t S = h->st.S, B = h->st.B;
        uint16_t code = 0;
        HIPCHK(h, hipMemcpy(&code, h->st.ordS + doc * S + i, 2, hipMemcpyDeviceToHost));
        std::vector<uint16_t> ob((size_t)MT_LV * B);
        HIPCHK(h, hipMemcpy(ob.data(), h->st.ordB + doc * MT_LV * B, ob.size() * 2, hipMemcpyDeviceToHost));
        const int dep = hd.hdr.depth;
        out->ordinal[dep - 1] = code;
        int x = i;
        for (int l = 0; l + 1 < dep; l++) {
            int b_ = 0, end = 0;
            while (b_ < hd.hdr.n_blk[l]) {
                end += hd.cnt[(size_t)l * B + b_];
                if (end > x) break;
                b_++;
            }
            out->ordinal[dep - 2 - l] = ob[(size_t)l * B + b_];
            x = b_;
        }
        out->ordinal_len = dep;
    } else if (h->ordinals && h->st.pgOS) {
        // paged: the slot's character, its leaf block's (page metadata), then the upper levels'
        // by position (level 1: the page's directory position; mt_paged.h "segment ordinals")
        const PagedBase pb = host_paged(h, doc);
        const size_t PP = pb.PP;
        const int pg = hd.rpage[i], slot = hd.rslot[i], dep = hd.hdr.depth;
        uint16_t code = 0;
        HIPCHK(h, hipMemcpy(&code, pb.oS + (size_t)pg * MT_PG_SLOTS + slot, 2, hipMemcpyDeviceToHost));
        out->ordinal[dep - 1] = code;
        if (dep >= 2) {
            const PageMeta &m = hd.pmeta[pg];
            int q = 0, st = 0;
            while (q + 1 < m.nblk && slot >= st + pm_bcnt(m, q)) st += pm_bcnt(m, q++);
            HIPCHK(h, hipMemcpy(&code, pb.oL + (size_t)pg * MT_PG_OLB + q, 2, hipMemcpyDeviceToHost));
            out->ordinal[dep - 2] = code;
        }
        if (dep >= 3) {
            std::vector<uint16_t> ou((size_t)MT_LV * PP);
            std::vector<uint8_t> cn((size_t)MT_LV * PP);
            HIPCHK(h, hipMemcpy(ou.data(), pb.oU, ou.size() * 2, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(cn.data(), pb.cnt, cn.size(), hipMemcpyDeviceToHost));
            int x = hd.rpos[i];
            out->ordinal[dep - 3] = ou[PP + x];
            for (int l = 2; l + 1 < dep; l++) {
                int b_ = 0, end = 0;
                while (b_ < hd.hdr.n_blk[l]) {
                    end += cn[(size_t)l * PP + b_];
                    if (end > x) break;
                    b_++;
                }
                out->ordinal[dep - 2 - l] = ou[(size_t)l * PP + b_];
                x = b_;
            }
        }
        out->ordinal_len = dep;
    }
    return 0;
}

// searchBlock (:1830-1862) for pos in view v: at every level the first child with
// pos < nodeLength(child), interior children by their partial lengths; no backtracking (a block
// whose leaves do not hold pos yields no segment).  The row (-1: none) and the offset into it.
static int host_search(const HostDoc &hd, const HostView &v, const HostTree &t, int pos, int &offset) {
    if (hd.hdr.n_seg == 0 || hd.lv.empty()) return -1;
    const int D = (int)hd.lv.size();
    int b = 0;
    for (int l = D - 1; l >= 1; l--) {
        int hit = -1;
        for (int k = t.first[l][b]; k < t.first[l][b] + hd.lv[l][b]; k++) {
            if (pos < t.P[l - 1][k]) {
                hit = k;
                break;
            }
            pos -= t.P[l - 1][k];
        }
        if (hit < 0) return -1;
        b = hit;
    }
    for (int i = t.first[0][b]; i < t.first[0][b] + hd.lv[0][b] && i < hd.hdr.n_seg; i++) {
        const int l = host_view_len(hd, v, i);
        if (pos < l) {
            offset = pos;
            return i;
        }
        pos -= l;
    }
    return -1;
}

// nodeMap (:2936-2998) in view v over the tree's partial lengths: a child -- interior by P, a
// leaf by its nodeLength -- is entered when (end > 0) && (len > 0) && (start < len) holds on the
// start and end shifted by the lengths before it, interior lengths included as they are (a block
// holding a row that is removed but not inserted in the view is shorter than its visible leaves,
// may be skipped outright, and shifts every later position).  The leaf action's arguments.
struct HostVisit {
    int row, pos, start, end;
};
static void host_map(const HostDoc &hd, const HostView &v, const HostTree &t, int l, int b, int &pos, int &start,
                     int &end, std::vector<HostVisit> &out) {
    for (int k = t.first[l][b]; k < t.first[l][b] + hd.lv[l][b]; k++) {
        if (l == 0 ? k >= hd.hdr.n_seg : k >= (int)t.P[l - 1].size()) break;
        const int len = l == 0 ? host_view_len(hd, v, k) : t.P[l - 1][k];
        if (end > 0 && len > 0 && start < len) {
            if (l == 0) {
                out.push_back(HostVisit{k, pos, start, end});
            } else {
                int p = pos, s = start, e = end;
                host_map(hd, v, t, l - 1, k, p, s, e, out);
            }
        }
        pos += len;
        start -= len;
        end -= len;
    }
}
static int walk_on_host(mt_handle *h, std::vector<uint32_t> todo, const uint32_t *docs, const int32_t *start,
                        const int32_t *end, const int32_t *ref_seq, const int32_t *client, uint32_t what,
                        std::vector<HostWalk> &out) {
    auto doc_of = [&](uint32_t q) { return docs ? docs[q] : q; };
    std::stable_sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) {
        if (doc_of(a) != doc_of(b)) return doc_of(a) < doc_of(b);
        if (client[a] != client[b]) return client[a] < client[b];
        return ref_seq[a] < ref_seq[b];
    });
    HostDoc hd;
    HostView v{0, 0, 0, false};
    HostTree t;
    int64_t have = -1, have_c = 0, have_r = 0;
    std::vector<HostVisit> vis;
    for (uint32_t q : todo) {
        const uint32_t d = doc_of(q);
        int rc;
        bool fresh = false;
        if ((int64_t)d != have) {
            if ((rc = fetch_doc(h, d, hd, (what & MT_WALK_TEXT) != 0u, (what & MT_WALK_PROPS) != 0u))) return rc;
            have = d;
            fresh = true;
        }
        if (fresh || client[q] != have_c || ref_seq[q] != have_r) {
            if ((rc = host_view_setup(h, d, hd, ref_seq[q], client[q], v))) return rc;
            host_tree(hd, v, t);
            have_c = client[q];
            have_r = ref_seq[q];
        }
        out.emplace_back();
        HostWalk &w = out.back();
        w.q = q;
        vis.clear();
        if (hd.hdr.n_seg > 0 && !hd.lv.empty()) {
            const int D = (int)hd.lv.size();
            int pos = 0, s = start ? start[q] : 0;
            int e = end && end[q] >= 0 ? end[q] : t.P[D - 1][0];   // an undefined end: blockLength(root)
            host_map(hd, v, t, D - 1, 0, pos, s, e, vis);
        }
        const uint32_t P = (uint32_t)(hd.props.size() / MT_PREC);
        for (const HostVisit &x : vis) {
            const int4 a = hd.A[x.row];
            const uint4 b = hd.B[x.row];
            const bool marker = (b.z & MT_MARKER_BIT) != 0u;
            mt_walk_row r;
            r.row = x.row;
            r.uid = b.z & ~MT_MARKER_BIT;
            r.position = x.pos;
            r.length = a.x;
            r.seq = a.y >= MT_LOCAL_BASE ? -1 : a.y;
            r.client = (int)(short)(a.w & 0xFFFF);
            r.marker_ref_type = marker ? (int32_t)b.x : -1;
            r.text = r.props = MT_PROPS_NONE;
            r.start = x.start;
            r.end = x.end;
            r.flags = MT_WALK_HOST;
            if ((what & MT_WALK_TEXT) && !marker && a.x > 0) {
                r.text = (uint32_t)w.text.size();
                for (int j = 0; j < a.x; j++) {
                    const size_t ix = (size_t)b.x + j;
                    w.text.push_back(ix < hd.text.size() ? hd.text[ix] : (uint16_t)0);
                }
            }
            if ((what & MT_WALK_PROPS) && b.y != 0u && b.y < P && hd.props[(size_t)b.y * MT_PREC] <= (uint32_t)MT_KMAX) {
                const uint32_t *x0 = hd.props.data() + (size_t)b.y * MT_PREC;
                r.props = (uint32_t)w.recs.size();
                w.recs.push_back(x0[0]);
                for (uint32_t k = 1; k < 1 + 2 * x0[0]; k++) w.recs.push_back(x0[k]);
            }
            w.rows.push_back(r);
        }
    }
    return 0;
}

int mt_get_containing_segment(mt_handle *h, uint32_t doc, int32_t pos, int32_t ref_seq, int32_t client,
                              mt_seg_info *out, uint16_t *text, uint32_t text_cap) {
    if (!out) return MT_E_INVALID;
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, text != nullptr, false);
    if (rc) return rc;
    HostView v;
    if ((rc = host_view_setup(h, doc, hd, ref_seq, client, v))) return rc;
    memset(out, 0, sizeof(*out));
    out->row = -1;
    if (hd.hdr.n_seg == 0 || hd.lv.empty()) return 0;
    HostTree t;
    host_tree(hd, v, t);
    int offset = 0;
    const int i = host_search(hd, v, t, pos, offset);
    if (i < 0) return 0;
    host_seg_info(h, doc, hd, i, out, text, text_cap);
    out->position = host_position(hd, v, t, i);
    out->offset = offset;
    return 0;
}

int mt_get_segment_by_uid(mt_handle *h, uint32_t doc, uint32_t uid, int32_t ref_seq, int32_t client,
                          mt_seg_info *out, uint16_t *text, uint32_t text_cap) {
    if (!out) return MT_E_INVALID;
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, text != nullptr, false);
    if (rc) return rc;
    HostView v;
    if ((rc = host_view_setup(h, doc, hd, ref_seq, client, v))) return rc;
    memset(out, 0, sizeof(*out));
    out->row = -1;
    for (int i = 0; i < hd.hdr.n_seg; i++) {
        if ((hd.B[i].z & ~MT_MARKER_BIT) == uid) {
            HostTree t;
            host_tree(hd, v, t);
            host_seg_info(h, doc, hd, i, out, text, text_cap);
            out->position = host_position(hd, v, t, i);
            return 0;
        }
    }
    return 0;
}

int mt_get_view_lengths(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *ref_seq,
                        const int32_t *client, int32_t *out) {
    if (!h || (n && (!docs || !ref_seq || !client || !out))) return MT_E_INVALID;
    HostDoc hd;
    int64_t have = -1;   // the document fetched last (queries of one document fetch it once)
    for (uint32_t q = 0; q < n; q++) {
        int rc;
        if ((int64_t)docs[q] != have) {
            if ((rc = fetch_doc(h, docs[q], hd, false, false))) return rc;
            have = docs[q];
        }
        HostView v;
        if ((rc = host_view_setup(h, docs[q], hd, ref_seq[q], client[q], v))) return rc;
        // blockLength(root) (:1664-1670): the root's partial length in a remote view
        int len = 0;
        for (int i = 0; i < hd.hdr.n_seg; i++) len += host_seg_partial(hd, v, i);
        out[q] = len;
    }
    return 0;
}

// ---------------------------------------------------------------- bulk segment read-outs
// mt_locate_segments / mt_locate_uids / mt_get_view_lengths_bulk / mt_resolve_remote_positions:
// one k_locate launch; the per-query marks come back with the view lengths (aux), and the
// queries the kernel marked MT_LOC_HOST are answered here from the single-query calls' code,
// grouped so that each document is fetched once and each view's tree built once.
namespace {
enum { LOC_POS = 0, LOC_UID = 1, LOC_LEN = 2 };
}
static int locate(mt_handle *h, const char *name, int mode, uint32_t n, const uint32_t *docs, const int32_t *key,
                  const int32_t *ref_seq, const int32_t *client, mt_seg_hit *out, void *out_dev, bool device,
                  std::vector<int4> *aux_out) {
    if (!h) return MT_E_INVALID;
    if (n && mode != LOC_LEN && (!key || (device ? !out_dev : !out))) return MT_E_INVALID;
    if ((ref_seq == nullptr) != (client == nullptr)) return MT_E_INVALID;
    const int bad = check_queries(h, name, n, docs);
    if (bad) return bad;
    for (uint32_t q = 0; mode == LOC_POS && q < n; q++)
        if (key[q] < 0) {
            h->err = std::string(name) + ": query " + std::to_string(q) + ": negative position";
            return MT_E_INVALID;
        }
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    ReadTimer &tm = h->tm_loc;
    tm.timed = 0;
    h->loc_n = n;
    h->loc_host = 0;
    if (aux_out) aux_out->clear();
    if (n == 0) return 0;
    QueryCols qc;   // extra: aux[n] (16 bytes each), the records (host results)
    const size_t aux_b = (size_t)n * sizeof(int4), hit_b = mode != LOC_LEN && !device ? (size_t)n * sizeof(mt_seg_hit) : 0;
    HIPCHK(h, qc.upload(n, {docs, key, ref_seq, client}, aux_b + hit_b));
    v4i *d_aux = (v4i *)qc.extra;
    mt_seg_hit *d_hit = device ? (mt_seg_hit *)out_dev : (mt_seg_hit *)(qc.extra + aux_b);
    const uint32_t *d_docs = (const uint32_t *)qc.col[0];
    const int32_t *d_key = (const int32_t *)qc.col[1], *d_ref = (const int32_t *)qc.col[2],
                  *d_cli = (const int32_t *)qc.col[3];
    // MT_LOCATE_ROW_WALK=1: observer-view queries walk every row (the A/B of tools/cursor_probe.py)
    const char *rw = getenv("MT_LOCATE_ROW_WALK");
    const int skip = !(rw && rw[0] == '1');
    HIPCHK(h, tm.begin(0, h->stream));
    if (mode == LOC_POS)
        hipLaunchKernelGGL(k_locate<0>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_key, d_ref, d_cli,
                           skip, d_hit, d_aux);
    else if (mode == LOC_UID)
        hipLaunchKernelGGL(k_locate<1>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_key, d_ref, d_cli,
                           skip, d_hit, d_aux);
    else
        hipLaunchKernelGGL(k_locate<2>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_key, d_ref, d_cli,
                           skip, (mt_seg_hit *)nullptr, d_aux);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(0, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    tm.timed = 1;
    std::vector<int4> aux(n);
    HIPCHK(h, hipMemcpy(aux.data(), d_aux, aux_b, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < n; q++)
        if (aux[q].x == MT_LOC_INVALID) {
            h->err = std::string(name) + ": query " + std::to_string(q) + ": remote view of document " +
                     std::to_string(docs ? docs[q] : q) + " with refSeq " + std::to_string(ref_seq[q]) +
                     " outside the collab window [minSeq, currentSeq]";
            return MT_E_INVALID;
        }
    if (hit_b) HIPCHK(h, hipMemcpy(out, d_hit, hit_b, hipMemcpyDeviceToHost));
    // the host path
    std::vector<uint32_t> todo;
    for (uint32_t q = 0; q < n; q++)
        if (aux[q].x == MT_LOC_HOST) todo.push_back(q);
    auto doc_of = [&](uint32_t q) { return docs ? docs[q] : q; };
    std::stable_sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) {
        if (doc_of(a) != doc_of(b)) return doc_of(a) < doc_of(b);
        if (client[a] != client[b]) return client[a] < client[b];
        return ref_seq[a] < ref_seq[b];
    });
    HostDoc hd;
    HostView v{0, 0, 0, false};
    const HostView obs{0, 0, 0, true};
    HostTree t, tl;
    int64_t have = -1, have_c = 0, have_r = 0;
    for (uint32_t q : todo) {
        const uint32_t d = doc_of(q);
        int rc;
        bool fresh = false;
        if ((int64_t)d != have) {
            if ((rc = fetch_doc(h, d, hd, false, false))) return rc;
            host_tree(hd, obs, tl);
            have = d;
            fresh = true;
        }
        if (fresh || client[q] != have_c || ref_seq[q] != have_r) {
            if ((rc = host_view_setup(h, d, hd, ref_seq[q], client[q], v))) return rc;
            host_tree(hd, v, t);
            have_c = client[q];
            have_r = ref_seq[q];
        }
        mt_seg_hit rec;
        memset(&rec, 0, sizeof(rec));
        rec.row = -1;
        rec.flags = MT_HIT_HOST;
        int row = -1, off = 0;
        if (mode == LOC_POS) {
            row = host_search(hd, v, t, key[q], off);
        } else {
            for (int i = 0; i < hd.hdr.n_seg && row < 0; i++)
                if ((hd.B[i].z & ~MT_MARKER_BIT) == (uint32_t)key[q]) row = i;
        }
        if (row >= 0) {
            mt_seg_info si;
            memset(&si, 0, sizeof(si));
            if ((rc = host_seg_info(h, d, hd, row, &si, nullptr, 0))) return rc;
            rec.row = si.row;
            rec.uid = si.uid;
            rec.position = host_position(hd, v, t, row);
            rec.offset = off;
            rec.local_position = host_position(hd, obs, tl, row);
            rec.length = si.length;
            rec.seq = si.seq;
            rec.client = si.client;
            rec.removed_seq = si.removed_seq;
            rec.removed_client = si.removed_client;
            rec.marker_ref_type = si.marker_ref_type;
        }
        if (device)
            HIPCHK(h, hipMemcpy((mt_seg_hit *)out_dev + q, &rec, sizeof(rec), hipMemcpyHostToDevice));
        else
            out[q] = rec;
    }
    h->loc_host = (int64_t)todo.size();
    if (aux_out) *aux_out = std::move(aux);
    return 0;
}

int mt_locate_segments(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *pos, const int32_t *ref_seq,
                       const int32_t *client, mt_seg_hit *out) {
    return locate(h, "mt_locate_segments", LOC_POS, n, docs, pos, ref_seq, client, out, nullptr, false, nullptr);
}
int mt_locate_uids(mt_handle *h, uint32_t n, const uint32_t *docs, const uint32_t *uids, const int32_t *ref_seq,
                   const int32_t *client, mt_seg_hit *out) {
    return locate(h, "mt_locate_uids", LOC_UID, n, docs, (const int32_t *)uids, ref_seq, client, out, nullptr, false,
                  nullptr);
}
int mt_locate_segments_device(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *pos,
                              const int32_t *ref_seq, const int32_t *client, void *out_dev) {
    return locate(h, "mt_locate_segments_device", LOC_POS, n, docs, pos, ref_seq, client, nullptr, out_dev, true,
                  nullptr);
}
int mt_locate_uids_device(mt_handle *h, uint32_t n, const uint32_t *docs, const uint32_t *uids, const int32_t *ref_seq,
                          const int32_t *client, void *out_dev) {
    return locate(h, "mt_locate_uids_device", LOC_UID, n, docs, (const int32_t *)uids, ref_seq, client, nullptr, out_dev,
                  true, nullptr);
}
int mt_get_view_lengths_bulk(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *ref_seq,
                             const int32_t *client, int32_t *out) {
    if (n && !out) return MT_E_INVALID;
    std::vector<int4> aux;
    const int rc = locate(h, "mt_get_view_lengths_bulk", LOC_LEN, n, docs, nullptr, ref_seq, client, nullptr, nullptr,
                          false, &aux);
    if (rc) return rc;
    for (uint32_t q = 0; q < n; q++) out[q] = aux[q].y;
    return 0;
}
int mt_resolve_remote_positions(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *pos,
                                const int32_t *ref_seq, const int32_t *client, int32_t *out) {
    if (n && !out) return MT_E_INVALID;
    std::vector<mt_seg_hit> hits(std::max<uint32_t>(n, 1));
    std::vector<int4> aux;
    const int rc = locate(h, "mt_resolve_remote_positions", LOC_POS, n, docs, pos, ref_seq, client, hits.data(), nullptr,
                          false, &aux);
    if (rc) return rc;
    // (aux: {mark, the view's length, the observer length when the walk found no segment})
    for (uint32_t q = 0; q < n; q++)
        out[q] = hits[q].row >= 0 ? hits[q].local_position + hits[q].offset : (pos[q] == aux[q].y ? aux[q].z : -1);
    return 0;
}
int mt_last_locate(mt_handle *h, int64_t *out, float *ms) {
    if (!h || !out) return MT_E_INVALID;
    out[0] = h->loc_n;
    out[1] = h->loc_host;
    float t[2] = {0.f, 0.f};
    if (ms) {
        const int rc = read_timer(h, h->tm_loc, t);
        *ms = t[0];
        if (rc) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------- bulk marker queries
// mt_find_tiles / mt_find_markers_by_id: one k_tiles launch.  Everything invalid is refused here,
// before the launch; the kernel has no host path.
static int tiles(mt_handle *h, const char *name, int mode, uint32_t n, const uint32_t *docs, const int32_t *pos,
                 const uint8_t *preceding, const uint32_t *label, uint32_t key, uint32_t n_labels,
                 const uint32_t *label_off, const uint32_t *label_vals, const uint32_t *id_val, mt_seg_hit *out,
                 void *out_dev, bool device) {
    if (!h) return MT_E_INVALID;
    if (h->live) {
        h->err = std::string(name) + ": not built for live handles";
        return MT_E_INVALID;
    }
    if (n && (device ? !out_dev : !out)) return MT_E_INVALID;
    if (n && (mode == 0 ? (!pos || !label) : !id_val)) return MT_E_INVALID;
    if (mode == 0 && (!label_off || (n_labels && label_off[n_labels] && !label_vals))) return MT_E_INVALID;
    const int bad = check_queries(h, name, n, docs);
    if (bad) return bad;
    if (mode == 0) {
        // the label table: offsets ascending from 0, every set strictly ascending plain ids
        if (label_off[0] != 0u) {
            h->err = std::string(name) + ": label offsets do not start at 0";
            return MT_E_INVALID;
        }
        for (uint32_t l = 0; l < n_labels; l++) {
            if (label_off[l + 1] < label_off[l]) {
                h->err = std::string(name) + ": label " + std::to_string(l) + ": offsets are not monotonic";
                return MT_E_INVALID;
            }
            for (uint32_t j = label_off[l]; j < label_off[l + 1]; j++) {
                const uint32_t v = label_vals[j];
                if (v == MT_VAL_NULL || v == MT_VAL_UNDEF || (v & (MT_VAL_FALSY_BIT | MT_VAL_NOMATCH_BIT))) {
                    h->err = std::string(name) + ": label " + std::to_string(l) + ": value id " + std::to_string(v) +
                             " carries flag bits or is null / undefined";
                    return MT_E_INVALID;
                }
                if (j > label_off[l] && label_vals[j - 1] >= v) {
                    h->err = std::string(name) + ": label " + std::to_string(l) + ": value ids are not sorted";
                    return MT_E_INVALID;
                }
            }
        }
        for (uint32_t q = 0; q < n; q++) {
            if (pos[q] < -1) {
                h->err = std::string(name) + ": query " + std::to_string(q) + ": position below -1 (undefined)";
                return MT_E_INVALID;
            }
            if (label[q] >= n_labels) {
                h->err = std::string(name) + ": query " + std::to_string(q) + ": no label " + std::to_string(label[q]);
                return MT_E_INVALID;
            }
        }
    }
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    ReadTimer &tm = h->tm_tile;
    tm.timed = 0;
    h->tile_n = n;
    h->tile_rows = 0;
    if (n == 0) return 0;
    // sel: label index | preceding << 31 (tiles), the id's value id (by id; flag bits dropped)
    std::vector<uint32_t> sel(n);
    for (uint32_t q = 0; q < n; q++)
        sel[q] = mode == 0 ? (label[q] | ((!preceding || preceding[q]) ? 0x80000000u : 0u))
                           : (id_val[q] == MT_VAL_NULL ? MT_VAL_NULL : id_val[q] & ~(MT_VAL_FALSY_BIT | MT_VAL_NOMATCH_BIT));
    // extra: examined[n], the label table (offsets, values), the records (host results)
    const size_t up8 = 7;
    const size_t ex_b = ((size_t)n * 4 + up8) & ~up8;
    const size_t off_b = mode == 0 ? (((size_t)n_labels + 1) * 4 + up8) & ~up8 : 0;
    const size_t val_b = mode == 0 ? ((size_t)label_off[n_labels] * 4 + up8) & ~up8 : 0;
    const size_t hit_b = device ? 0 : (size_t)n * sizeof(mt_seg_hit);
    QueryCols qc;
    HIPCHK(h, qc.upload(n, {docs, pos, sel.data()}, hit_b + ex_b + off_b + val_b));
    mt_seg_hit *d_hit = device ? (mt_seg_hit *)out_dev : (mt_seg_hit *)qc.extra;
    int32_t *d_ex = (int32_t *)(qc.extra + hit_b);
    uint32_t *d_off = (uint32_t *)(qc.extra + hit_b + ex_b), *d_val = (uint32_t *)(qc.extra + hit_b + ex_b + off_b);
    if (mode == 0) {
        HIPCHK(h, hipMemcpy(d_off, label_off, ((size_t)n_labels + 1) * 4, hipMemcpyHostToDevice));
        if (label_off[n_labels])
            HIPCHK(h, hipMemcpy(d_val, label_vals, (size_t)label_off[n_labels] * 4, hipMemcpyHostToDevice));
    }
    const uint32_t *d_docs = (const uint32_t *)qc.col[0], *d_sel = (const uint32_t *)qc.col[2];
    const int32_t *d_pos = (const int32_t *)qc.col[1];
    // MT_LOCATE_ROW_WALK=1: walk from row 0 (the A/B of tools/tile_probe.py)
    const char *rw = getenv("MT_LOCATE_ROW_WALK");
    const int skip = !(rw && rw[0] == '1');
    HIPCHK(h, tm.begin(0, h->stream));
    if (mode == 0)
        hipLaunchKernelGGL(k_tiles<0>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_pos, d_sel, key, d_off,
                           d_val, skip, d_hit, d_ex);
    else
        hipLaunchKernelGGL(k_tiles<1>, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_pos, d_sel, key,
                           (const uint32_t *)nullptr, (const uint32_t *)nullptr, skip, d_hit, d_ex);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(0, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    tm.timed = 1;
    std::vector<int32_t> ex(n);
    HIPCHK(h, hipMemcpy(ex.data(), d_ex, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < n; q++) h->tile_rows += ex[q];
    if (hit_b) HIPCHK(h, hipMemcpy(out, d_hit, hit_b, hipMemcpyDeviceToHost));
    return 0;
}
int mt_find_tiles(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *pos, const uint8_t *preceding,
                  const uint32_t *label, uint32_t tile_key, uint32_t n_labels, const uint32_t *label_off,
                  const uint32_t *label_vals, mt_seg_hit *out) {
    return tiles(h, "mt_find_tiles", 0, n, docs, pos, preceding, label, tile_key, n_labels, label_off, label_vals, nullptr,
                 out, nullptr, false);
}
int mt_find_tiles_device(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *pos, const uint8_t *preceding,
                         const uint32_t *label, uint32_t tile_key, uint32_t n_labels, const uint32_t *label_off,
                         const uint32_t *label_vals, void *out_dev) {
    return tiles(h, "mt_find_tiles_device", 0, n, docs, pos, preceding, label, tile_key, n_labels, label_off, label_vals,
                 nullptr, nullptr, out_dev, true);
}
int mt_find_markers_by_id(mt_handle *h, uint32_t n, const uint32_t *docs, uint32_t id_key, const uint32_t *id_val,
                          mt_seg_hit *out) {
    return tiles(h, "mt_find_markers_by_id", 1, n, docs, nullptr, nullptr, nullptr, id_key, 0, nullptr, nullptr, id_val, out,
                 nullptr, false);
}
int mt_find_markers_by_id_device(mt_handle *h, uint32_t n, const uint32_t *docs, uint32_t id_key, const uint32_t *id_val,
                                 void *out_dev) {
    return tiles(h, "mt_find_markers_by_id_device", 1, n, docs, nullptr, nullptr, nullptr, id_key, 0, nullptr, nullptr,
                 id_val, nullptr, out_dev, true);
}
int mt_last_tiles(mt_handle *h, int64_t *out, float *ms) {
    if (!h || !out) return MT_E_INVALID;
    out[0] = h->tile_n;
    out[1] = h->tile_rows;
    float t[2] = {0.f, 0.f};
    if (ms) {
        const int rc = read_timer(h, h->tm_tile, t);
        *ms = t[0];
        if (rc) return rc;
    }
    return 0;
}

// Debug: raw segment records (segA, segB as 8 u32 per segment) and header words.
int mt_debug_raw(mt_handle *h, uint32_t doc, uint32_t *rows, uint32_t cap_rows, uint32_t *n_rows,
                 int32_t *hdr_words) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, false);
    if (rc) return rc;
    const int n = hd.hdr.n_seg;
    for (int i = 0; i < n && rows && (uint32_t)i < cap_rows; i++) {
        memcpy(rows + 8 * i, &hd.A[i], 16);
        memcpy(rows + 8 * i + 4, &hd.B[i], 16);
        rows[8 * i + 7] &= ~SEGF_PSIG_MASK;   // the signature bits stay on the device
    }
    if (n_rows) *n_rows = (uint32_t)n;
    if (hdr_words) memcpy(hdr_words, &hd.hdr, sizeof(DocHdr));
    return 0;
}

// Debug: the property-set signature each row carries (the bits no other read-out returns).
int mt_debug_props_sigs(mt_handle *h, uint32_t doc, uint32_t *sigs, uint32_t cap_rows, uint32_t *n_rows) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, false);
    if (rc) return rc;
    const int n = hd.hdr.n_seg;
    for (int i = 0; i < n && sigs && (uint32_t)i < cap_rows; i++) sigs[i] = psig_of(hd.B[i].w);
    if (n_rows) *n_rows = (uint32_t)n;
    return 0;
}

uint32_t mt_props_signature(const uint32_t *pairs, int n) {
    uint32_t sig = 0;
    for (int j = 0; j < n; j++) sig += mt_psig_mix(pairs[2 * j], pairs[2 * j + 1]);
    return sig & 0xFFFu;
}

// Debug (flat documents): the zamboni heap in array order as {maxSeq, leaf index of its
// segment or -1} and the leaf blocks' needsScour flags.
int mt_debug_heap(mt_handle *h, uint32_t doc, int32_t *heap, uint32_t cap, uint32_t *n_heap, int32_t *flags,
                  uint32_t cap_flags, uint32_t *n_flags) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, false);
    if (rc) return rc;
    if (hd.hdr.pad[HDR_PAGED]) return MT_E_INVALID;
    const DevState &st = h->st;
    std::vector<int2> hp((size_t)st.H + 1);
    std::vector<int8_t> fl((size_t)st.B);
    HIPCHK(h, hipMemcpy(hp.data(), st.heap + doc * (size_t)(st.H + 1), hp.size() * sizeof(int2), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(fl.data(), st.flg + doc * (size_t)st.B, fl.size(), hipMemcpyDeviceToHost));
    const int n = hd.hdr.n_seg;
    for (int k = 1; k <= hd.hdr.heap_n && (uint32_t)(k - 1) < cap; k++) {
        int at = -1;
        for (int i = 0; i < n; i++)
            if ((hd.B[i].z & ~MT_MARKER_BIT) == (uint32_t)hp[k].y) at = i;
        heap[2 * (k - 1)] = hp[k].x;
        heap[2 * (k - 1) + 1] = at;
    }
    if (n_heap) *n_heap = (uint32_t)hd.hdr.heap_n;
    for (int b = 0; b < hd.hdr.n_blk[0] && (uint32_t)b < cap_flags; b++) flags[b] = fl[b];
    if (n_flags) *n_flags = (uint32_t)hd.hdr.n_blk[0];
    return 0;
}

int mt_get_overlap_arena(mt_handle *h, uint32_t doc, int32_t *out) {
    if (!out) return MT_E_INVALID;
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, false);
    if (rc) return rc;
    for (int k = 0; k < 7; k++) out[k] = 0;
    if (hd.ovf.size() < MT_OVF_HDR) return 0;
    uint32_t w[MT_OVF_HDR / 2];
    memcpy(w, hd.ovf.data(), sizeof(w));
    const int OA = (int)hd.ovf.size(), mid = mt_ovf_mid(OA);
    const int half = (w[3] & 1) && (int)w[0] > mid ? 1 : 0;
    out[0] = OA;
    out[1] = (int)w[0] - (half ? mid : MT_OVF_HDR);
    out[2] = half;
    out[3] = (int)w[2];
    std::vector<uint32_t> offs;
    for (int i = 0; i < hd.hdr.n_seg; i++)
        if (hd.O[i] & MT_OVF_BIT) offs.push_back((uint32_t)hd.O[i]);
    std::sort(offs.begin(), offs.end());
    offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
    for (uint32_t off : offs) out[4] += off < hd.ovf.size() ? (int)hd.ovf[off] + 1 : 0;
    out[5] = (int)std::min<uint32_t>(w[4], INT32_MAX);
    out[6] = (int)w[5];
    return 0;
}

int mt_get_segment_props(mt_handle *h, uint32_t doc, uint32_t seg_index, uint32_t *pairs,
                         uint32_t cap_pairs, int32_t *n_pairs) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, true);
    if (rc) return rc;
    if ((int)seg_index >= hd.hdr.n_seg) return MT_E_INVALID;
    const uint32_t ph = hd.B[seg_index].y;
    if (ph == 0) {
        *n_pairs = -1;
        return 0;
    }
    const uint32_t *x = &hd.props[(size_t)ph * MT_PREC];
    for (uint32_t k = 0; k < x[0] && k < cap_pairs; k++) {
        pairs[2 * k] = x[1 + 2 * k];
        pairs[2 * k + 1] = x[2 + 2 * k];
    }
    *n_pairs = (int32_t)x[0];
    return 0;
}

int mt_get_all_segment_props(mt_handle *h, uint32_t doc, int32_t *out, uint64_t cap_words, uint64_t *n_words) {
    HostDoc hd;
    int rc = fetch_doc(h, doc, hd, false, true);
    if (rc) return rc;
    uint64_t w = 0;
    for (int i = 0; i < hd.hdr.n_seg; i++) {
        const uint32_t ph = hd.B[i].y;
        const uint32_t *x = ph ? &hd.props[(size_t)ph * MT_PREC] : nullptr;
        const int np = x ? (int)x[0] : -1;
        if (out && w < cap_words) out[w] = np;
        w++;
        for (int k = 0; k < np; k++, w += 2)
            if (out && w + 1 < cap_words) {
                out[w] = (int32_t)x[1 + 2 * k];
                out[w + 1] = (int32_t)x[2 + 2 * k];
            }
    }
    if (n_words) *n_words = w;
    return 0;
}

int mt_get_delta_log(mt_handle *h, uint32_t doc, int32_t *out, uint32_t cap, uint32_t *n) {
    if (!h || doc >= h->n_docs) return MT_E_INVALID;
    if (!h->st.DL) {
        if (n) *n = 0;
        return 0;
    }
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    DocHdr hdr;
    HIPCHK(h, hipMemcpy(&hdr, h->st.hdr + doc, sizeof(DocHdr), hipMemcpyDeviceToHost));
    // only whole records are ever counted; clamp anyway (never read past this document)
    const uint32_t have = (uint32_t)std::min<int64_t>(std::max<int32_t>(hdr.dlog_n, 0), h->st.DL);
    const uint32_t cnt = std::min<uint32_t>(have, cap);
    if (out && cnt) HIPCHK(h, hipMemcpy(out, h->st.dlog + (size_t)doc * h->st.DL, cnt * 4, hipMemcpyDeviceToHost));
    if (n) *n = have;
    if (hdr.pad[HDR_DLOG_OVF]) {
        h->err = "mt_get_delta_log: document " + std::to_string(doc) +
                 " overflowed its delta log (delta_log_capacity) since the last mt_delta_log_reset";
        return MT_E_OVERFLOW;
    }
    return 0;
}

__global__ void __launch_bounds__(MT_WAVE) k_dlog_reset(DevState st) {
    const int doc = blockIdx.x * MT_WAVE + threadIdx.x;
    if (doc >= st.n_docs) return;
    st.hdr[doc].dlog_n = 0;
    st.hdr[doc].pad[HDR_DLOG_OVF] = 0;
}

int mt_delta_log_reset(mt_handle *h) {
    if (!h) return MT_E_INVALID;
    if (h->pending) SETTLE(h);
    if (!h->st.DL) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_dlog_reset, dim3((h->n_docs + MT_WAVE - 1) / MT_WAVE), dim3(MT_WAVE), 0, h->stream, h->st);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int mt_delta_log_reset_docs(mt_handle *h, uint32_t n, const uint32_t *docs) {
    if (!h) return MT_E_INVALID;
    const int bad = check_queries(h, "mt_delta_log_reset_docs", n, docs);
    if (bad) return bad;
    if (h->pending) SETTLE(h);
    if (!h->st.DL || n == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    if (docs) {   // the list lives in a buffer of the handle's: nothing to free behind the kernel
        if (n > h->rst_cap) {
            HIPCHK(h, hipStreamSynchronize(h->stream));   // (an earlier reset may still read the old one)
            if (h->d_rst) HIPCHK(h, hipFree(h->d_rst));
            h->d_rst = nullptr;
            h->rst_cap = 0;
            HIPCHK(h, hipMalloc((void **)&h->d_rst, (size_t)n * 4));
            h->rst_cap = n;
        }
        HIPCHK(h, hipMemcpyAsync(h->d_rst, docs, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(k_dlog_reset_docs, dim3((n + MT_WAVE - 1) / MT_WAVE), dim3(MT_WAVE), 0, h->stream, h->st, (int)n,
                       docs ? h->d_rst : (const uint32_t *)nullptr);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// mt_get_delta_logs / mt_get_delta_logs_device: get_prop_runs_bulk's shape -- the counting pass
// (words from the header, rows by the walk), one or two prefix sums, the gather.
static int get_delta_logs(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *from_word, int64_t *off,
                          int64_t *row_off, uint32_t *flags, void *out, uint64_t cap, void *rows, uint64_t cap_rows,
                          bool device) {
    if (!h || !off) return MT_E_INVALID;
    int rc = check_queries(h, "mt_get_delta_logs", n, docs);
    if (rc) return rc;
    for (uint32_t q = 0; from_word && q < n; q++)
        if (from_word[q] < 0) {
            h->err = "mt_get_delta_logs: query " + std::to_string(q) + ": from_word " + std::to_string(from_word[q]);
            return MT_E_INVALID;
        }
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    ReadTimer &tm = h->tm_dlg;
    tm.timed = 0;
    const int k = row_off ? 2 : 1;
    int64_t *offs[2] = {off, row_off};
    if (n == 0) {
        for (int i = 0; i < k; i++)
            if ((rc = empty_offsets(h, {offs[i]}, device))) return rc;
        return 0;
    }
    if (!h->st.DL) {   // no log: zero words and rows, as mt_get_delta_log answers
        for (int i = 0; i < k; i++)
            if (device)
                HIPCHK(h, hipMemset(offs[i], 0, ((size_t)n + 1) * 8));
            else
                memset(offs[i], 0, ((size_t)n + 1) * 8);
        if (flags && device) HIPCHK(h, hipMemset(flags, 0, (size_t)n * 4));
        if (flags && !device) memset(flags, 0, (size_t)n * 4);
        return 0;
    }
    // extra: the word and row counts [n] each, the two offset arrays [n + 1] each, the flags [n]
    const size_t words64 = (size_t)n * 4 + 2;
    QueryCols qc;
    HIPCHK(h, qc.upload(n, {docs, from_word}, words64 * 8 + (((size_t)n * 4 + 7) & ~(size_t)7)));
    const uint32_t *d_docs = (const uint32_t *)qc.col[0];
    const int32_t *d_from = (const int32_t *)qc.col[1];
    int64_t *d_cnt[2] = {(int64_t *)qc.extra, (int64_t *)qc.extra + n};   // words, rows
    int64_t *d_woff = device ? off : d_cnt[1] + n, *d_roff = device ? row_off : d_cnt[1] + 2 * (size_t)n + 1;
    uint32_t *d_flags = (uint32_t *)((int64_t *)qc.extra + words64);
    HIPCHK(h, tm.begin(0, h->stream));
    hipLaunchKernelGGL(k_dlog_count, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_from, k == 2 ? 1 : 0,
                       d_cnt[0], d_cnt[1], d_flags);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, tm.end(0, h->stream));
    int64_t total[2] = {0, 0};
    if ((rc = scan_counts(h, n, k, d_cnt, offs, device, total))) return rc;
    tm.timed = 1;
    // the flags: to the caller, and to the host when nobody else would see an overflow
    std::vector<uint32_t> own_flags;
    if (flags) HIPCHK(h, hipMemcpy(flags, d_flags, (size_t)n * 4, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    if (!flags) {
        own_flags.resize(n);
        HIPCHK(h, hipMemcpy(own_flags.data(), d_flags, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    if (!rows) cap_rows = 0;
    rc = after_counts(h, !out, cap >= (uint64_t)total[0] && (k == 1 || cap_rows >= (uint64_t)total[1]), total[0] == 0, [&] {
        return "mt_get_delta_logs: the outputs hold " + std::to_string(cap) + " words and " + std::to_string(cap_rows) +
               " rows, the results need " + std::to_string(total[0]) + " words and " + std::to_string(total[1]) + " rows";
    });
    if (rc < 0) return rc;
    if (rc == RO_GATHER) {
        if (!device) {
            HIPCHK(h, hipMemcpy(d_woff, off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
            if (k == 2) HIPCHK(h, hipMemcpy(d_roff, row_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
        }
        OutStage<int32_t> g_words;
        OutStage<mt_delta_range> g_rows;
        HIPCHK(h, g_words.open(out, device, (size_t)total[0]));
        if (k == 2) HIPCHK(h, g_rows.open(rows, device, (size_t)total[1]));
        HIPCHK(h, tm.begin(1, h->stream));
        hipLaunchKernelGGL(k_dlog_gather, dim3(n), dim3(MT_WAVE), 0, h->stream, h->st, (int)n, d_docs, d_from, d_woff,
                           k == 2 ? d_roff : (const int64_t *)nullptr, g_words.p, g_rows.p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, tm.end(1, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        tm.timed = 2;
        HIPCHK(h, g_words.copy_out(out, (size_t)total[0]));
        if (k == 2) HIPCHK(h, g_rows.copy_out(rows, (size_t)total[1]));
    }
    for (uint32_t q = 0; q < (uint32_t)own_flags.size(); q++)
        if (own_flags[q] & MT_DLOG_OVERFLOWED) {
            h->err = "mt_get_delta_logs: query " + std::to_string(q) + ": document " + std::to_string(docs ? docs[q] : q) +
                     " overflowed its delta log (delta_log_capacity) since its last reset";
            return MT_E_OVERFLOW;
        }
    return 0;
}

int mt_get_delta_logs(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *from_word, int64_t *off,
                      int64_t *row_off, uint32_t *flags, int32_t *out, uint64_t cap, mt_delta_range *rows,
                      uint64_t cap_rows) {
    return get_delta_logs(h, n, docs, from_word, off, row_off, flags, out, cap, rows, cap_rows, false);
}

int mt_get_delta_logs_device(mt_handle *h, uint32_t n, const uint32_t *docs, const int32_t *from_word, void *off_dev,
                             void *row_off_dev, void *flags_dev, void *out_dev, uint64_t cap, void *rows_dev,
                             uint64_t cap_rows) {
    return get_delta_logs(h, n, docs, from_word, (int64_t *)off_dev, (int64_t *)row_off_dev, (uint32_t *)flags_dev,
                          out_dev, cap, rows_dev, cap_rows, true);
}

int mt_last_dlog_ms(mt_handle *h, float *out) {
    if (!h || !out) return MT_E_INVALID;
    return read_timer(h, h->tm_dlg, out);
}

// Debug: section timers of an MT_PROF build (s_memtime ticks [0, 64) and call / event counts
// [64, 128)).
int mt_debug_pick(const mt_pick_query *q, char *name, uint32_t name_cap, uint64_t *lds_bytes) {
    if (!q || !name || !name_cap || !lds_bytes) return MT_E_INVALID;
    const HandleFacts f{q->delta_log != 0, q->ordinals != 0, q->live != 0, q->wpg};
    const TierCaps lds{q->S, q->B, q->H, 0, 0}, hbm{0, q->B, 0, 0, 0};
    const PagedCaps pc{q->PP, q->PH, q->UT, 0, 0, q->narrow, q->grow, q->packed};
    Pick p{nullptr, 0};
    switch (q->launch) {
    case MT_PICK_REPLAY_LDS: p = pick_flat(K_REPLAY, f, lds, 0); break;
    case MT_PICK_REPLAY_HBM: p = pick_flat(K_REPLAY, f, hbm, 0); break;
    case MT_PICK_REPLAY_PAGED: p = pick_paged(K_REPLAY_PAGED, f, pc, q->big != 0, 0); break;
    case MT_PICK_GENERATE_LDS: p = pick_flat(K_GENERATE, f, lds, q->gen_words); break;
    case MT_PICK_GENERATE_HBM: p = pick_flat(K_GENERATE, f, hbm, q->gen_words); break;
    case MT_PICK_GENERATE_PAGED: p = pick_paged(K_GENERATE_PAGED, f, pc, false, q->gen_words); break;
    case MT_PICK_LOAD_CONVERT: p = pick_paged(K_LOAD_CONVERT, f, pc, q->big != 0, 0); break;
    case MT_PICK_OCCUPANCY: p = pick_paged(K_REPLAY_PAGED, f, pc, false, 0, true); break;
    }
    if (!p.v) return MT_E_INVALID;
    snprintf(name, name_cap, "%s", p.v->name);
    *lds_bytes = p.lds;
    return 0;
}

int mt_debug_prof(mt_handle *h, uint64_t *out, int reset) {
#ifdef MT_PROF
    if (!h || !h->st.prof) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    if (out) HIPCHK(h, hipMemcpy(out, h->st.prof, 128 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(h, hipMemset(h->st.prof, 0, 128 * sizeof(uint64_t)));
    return 0;
#else
    (void)h; (void)out; (void)reset;
    return MT_E_INVALID;
#endif
}

int mt_checksums_device(mt_handle *h, void *device_out) {
    if (!h || !device_out) return MT_E_INVALID;
    if (h->pending) SETTLE(h);
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_checksum, dim3(h->n_docs), dim3(MT_WAVE), 0, h->stream, h->st,
                       (mt_checksum *)device_out);
    HIPCHK(h, hipGetLastError());
    SETTLE(h);
    return 0;
}

int mt_maintenance_counts(mt_handle *h, uint32_t *out) {
    if (!h || !out || !h->st.DL) return MT_E_INVALID;   // kept by delta-logging handles only
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    std::vector<DocHdr> hd(h->n_docs);
    HIPCHK(h, hipMemcpy(hd.data(), h->st.hdr, h->n_docs * sizeof(DocHdr), hipMemcpyDeviceToHost));
    for (uint32_t d = 0; d < h->n_docs; d++) {
        out[3 * d] = (uint32_t)hd[d].pad[HDR_MSPLIT];
        out[3 * d + 1] = (uint32_t)hd[d].pad[HDR_MAPPEND];
        out[3 * d + 2] = (uint32_t)hd[d].pad[HDR_MUNLINK];
    }
    return 0;
}

int mt_checksums(mt_handle *h, mt_checksum *out) {
    if (!h || !out) return MT_E_INVALID;
    int rc = mt_checksums_device(h, h->d_sums);
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(out, h->d_sums, h->n_docs * sizeof(mt_checksum), hipMemcpyDeviceToHost));
    return 0;
}

int mt_regenerate_pending(mt_handle *h, uint32_t doc, mt_regen_rec *out, uint32_t cap, int32_t *n_out,
                          uint16_t *out_text, uint32_t text_cap, uint32_t *out_props, uint32_t props_cap) {
    if (!h || !h->live || doc >= h->n_docs || !n_out || (cap && !out) || (text_cap && !out_text) ||
        (props_cap && !out_props)) {
        if (h) h->err = "mt_regenerate_pending: needs a live_client handle, a document and output buffers";
        return MT_E_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    DevBuf<mt_regen_rec> d_out;
    DevBuf<uint16_t> d_text;
    DevBuf<uint32_t> d_props;
    DevBuf<int32_t> d_io;
    HIPCHK(h, d_out.alloc(cap));
    HIPCHK(h, d_text.alloc(text_cap));
    HIPCHK(h, d_props.alloc(props_cap));
    HIPCHK(h, d_io.alloc(4));
    int32_t io[4] = {0, 0, 0, 0};
    for (int round = 0; round < 8; round++) {
        // the flat HBM tier's LDS (the B-tree counts), which the live growth step can raise
        const size_t lds = lds_layout(false, 0, h->st.B, 0, 0).total;
        HIPCHK(h, raise_lds_limit((const void *)k_regen, lds));
        hipLaunchKernelGGL(k_regen, dim3(1), dim3(MT_WAVE), lds, h->stream, h->st, (int)doc, d_out.p, (int)cap,
                           d_text.p, (int)text_cap, d_props.p, (int)props_cap, d_io.p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(io, d_io.p, 16, hipMemcpyDeviceToHost));
        if (io[0] != -5) break;
        // more segment groups than the handle's ring holds (nothing changed yet): grow it
        const int lg2 = std::min(65535, std::max(2 * h->st.LG, io[1]));
        if (lg2 <= h->st.LG || live_regrow(h, h->st.S, h->st.B, h->st.H, h->st.T, h->st.P, lg2) != 0) {
            io[0] = -2;
            break;
        }
    }
    if (io[0] > 0) {
        HIPCHK(h, hipMemcpy(out, d_out.p, (size_t)io[0] * sizeof(mt_regen_rec), hipMemcpyDeviceToHost));
        if (io[1]) HIPCHK(h, hipMemcpy(out_text, d_text.p, (size_t)io[1] * 2, hipMemcpyDeviceToHost));
        if (io[2]) HIPCHK(h, hipMemcpy(out_props, d_props.p, (size_t)io[2] * 4, hipMemcpyDeviceToHost));
    }
    if (io[0] == -3) {
        h->err = "mt_regenerate_pending: the document has failed";
        return MT_E_INVALID;
    }
    if (io[0] == -2) {
        h->err = "mt_regenerate_pending: capacity (group table or a segment's group FIFO); document failed";
        return MT_E_INVALID;
    }
    if (io[0] == -4) {   // nothing changed: retry with buffers of these sizes
        h->err = "mt_regenerate_pending: output buffers too small: need " + std::to_string(io[1]) + " records, " +
                 std::to_string(io[2]) + " text units, " + std::to_string(io[3]) + " props words";
        *n_out = -2;
        return MT_E_OVERFLOW;
    }
    *n_out = io[0];
    return 0;
}

int mt_pending_counts(mt_handle *h, int32_t *out) {
    if (!h || !h->live || !out) return MT_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    SETTLE(h);
    std::vector<int32_t> lv((size_t)h->n_docs * 4);
    HIPCHK(h, hipMemcpy(lv.data(), h->st.live, lv.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t d = 0; d < h->n_docs; d++) {
        out[2 * d] = lv[4 * d];
        out[2 * d + 1] = lv[4 * d + 2];
    }
    return 0;
}

}  // extern "C"
