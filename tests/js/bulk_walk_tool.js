"use strict";
// Test driver for the Node facade's segment walk (fluidframework_amd/js).  Usage:
//   node tests/js/bulk_walk_tool.js <ref_walk fixture.json.gz> <flushEvery (0: one flush)>
// Replays the fixture through GpuClients, then prints JSON per document for its final checkpoint:
//   walks   per query of the checkpoint: what GpuClient.walkSegments handed the handler, one
//           [pos, start, end, cachedLength, seq, clientId, text | null, refType | null,
//           property entries in key order | null] per visit
//   args    {checked, ok}: refSeq / clientId / accum as the handler received them
//   stops   [[k, visits]]: handlers that return false at their k-th call
//   same    {checked, ok}: the visited segment is getContainingSegment(pos).segment (one object
//           per segment), on a sample of the visits
//   tam     per label [parallelText, [[refType, property entries] per marker]]
//   extents [[pos, posStart | null, posAfterEnd | null]]
//   batch   true when one GpuMergeTreeBatch.walkSegments call for all queries of all documents
//           gave the same visits and the same segment objects as the per-client calls
//   split   the message of the splitRange throw
// The fixture was produced by the reference itself (tests/golden/make_walk.py).
const fs = require("fs");
const zlib = require("zlib");
const path = require("path");
const repo = path.join(__dirname, "..", "..");

function msgs(doc) {
    return doc.msgs.map((rec) => ({
        clientId: `client-${rec[0]}`, sequenceNumber: rec[1], referenceSequenceNumber: rec[2],
        minimumSequenceNumber: rec[3], contents: rec[4], type: rec.length > 5 ? rec[5] : "op",
    }));
}
const entries = (p) => (p === undefined ? null : Object.entries(p));
const nul = (v) => (v === undefined ? null : v);

const [file, every] = process.argv.slice(2);
const flushEvery = parseInt(every, 10);
const fx = JSON.parse(zlib.gunzipSync(fs.readFileSync(file)).toString("utf8"));
const { GpuMergeTreeBatch } = require(path.join(repo, "fluidframework_amd", "js"));
const batch = new GpuMergeTreeBatch(fx.docs.length, { segCapacity: 8192, textCapacity: 1 << 17, deltaLogCapacity: 1 << 20 });
batch.loadInitialText(fx.docs.map((d) => d.seed_text));
const views = fx.docs.map((d, i) => {
    const c = batch.client(i);
    c.startOrUpdateCollaboration("observer");
    return c;
});
const all = fx.docs.map(msgs);
const longest = Math.max(...all.map((m) => m.length));
for (let at = 0; at < longest; at += flushEvery || longest) {
    all.forEach((m, i) => { for (const x of m.slice(at, at + (flushEvery || longest))) { views[i].applyMsg(x); } });
    batch.flush();
}
const last = fx.docs.map((d) => d.checkpoints[d.checkpoints.length - 1]);
const und = (v) => (v === null ? undefined : v);
const out = [];
const seen = [];          // per document, per query: the segment objects visited
const bq = [];
last.forEach((cp, i) => {
    const c = views[i];
    const o = { walks: [], args: { checked: 0, ok: 0 }, stops: [], same: { checked: 0, ok: 0 }, tam: [], extents: [] };
    const objs = [];
    cp.walks.forEach(([start, end], k) => {
        const visits = [], segs = [], accum = { k };
        c.walkSegments((seg, pos, refSeq, clientId, s, e, acc) => {
            visits.push([pos, s, e, seg.cachedLength, seg.seq, seg.clientId, nul(seg.text), nul(seg.refType), entries(seg.properties)]);
            segs.push(seg);
            o.args.checked++;
            if (refSeq === c.getCurrentSeq() && clientId === 0 && acc === accum) { o.args.ok++; }
            return true;
        }, und(start), und(end), accum);
        o.walks.push(visits);
        objs.push(segs);
        bq.push({ doc: i, start: und(start), end: und(end) });
        if (k < 4) {
            for (const stopAt of [1, 3]) {
                let n = 0;
                c.walkSegments(() => { n++; return n < stopAt; }, und(start), und(end));
                o.stops.push([stopAt, n, visits.length]);
            }
        }
        if (k % 5 === 0) {
            visits.forEach((v, j) => {
                if (j % 9 !== 0) { return; }
                o.same.checked++;
                const r = c.getContainingSegment(v[0]);
                if (r.segment === segs[j] && r.offset === 0) { o.same.ok++; }
            });
        }
    });
    seen.push(objs);
    for (const label of fx.labels) {
        const r = c.getTextAndMarkers(label);
        o.tam.push([r.parallelText, r.parallelMarkers.map((m) => [m.refType, entries(m.properties)])]);
    }
    for (const [pos] of cp.extents) {
        const r = c.getRangeExtentsOfPosition(pos);
        o.extents.push([pos, nul(r.posStart), nul(r.posAfterEnd)]);
    }
    out.push(o);
});
const bulk = batch.walkSegments(bq);
let same = bulk.length === bq.length, at = 0;
last.forEach((cp, i) => {
    cp.walks.forEach((_, k) => {
        const rows = bulk[at++], v = out[i].walks[k], segs = seen[i][k];
        same = same && rows.length === v.length && rows.every((r, j) => r.pos === v[j][0] && r.start === v[j][1] &&
            r.end === v[j][2] && r.segment === segs[j]);
    });
});
let split = null;
try { views[0].walkSegments(() => true, 0, 1, undefined, true); } catch (e) { split = e.message; }
process.stdout.write(JSON.stringify({ docs: out, batch: same, split }));
