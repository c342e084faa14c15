"use strict";
// Test driver for the Node facade's walk in a (refSeq, client) view (fluidframework_amd/js).  Usage:
//   node tests/js/view_walk_tool.js <docs.json>
// docs.json: [{doc, seed_text, msgs, views: [{refSeq, client, walks: [[start | null, end | null]],
// texts: [[walk index, placeholder]]}]}] -- the fixture's final checkpoints (tests/test_js_view_walk.py
// writes it).  Replays the documents through GpuClients and prints JSON per document:
//   walks   per view, per query: what mergeTree.mapRange handed the leaf action, one [pos, start,
//           end, cachedLength, seq, clientId, text | null, refType | null] per visit
//   args    {checked, ok}: refSeq / clientId / accum as the leaf action received them
//   clones  per view: cloneSegments(refSeq, client, start, end) of the view's first query as
//           [cachedLength, text | null] per segment, and whether every clone is a new object
//   texts   per view: getTextInView(refSeq, client, placeholder, start, end) per asked query
//   stops   [[k, visits, total]]: leaf actions that return false at their k-th call
//   throws  the messages of the throws: pre / post / shift / contains actions, splitRange, "*"
const fs = require("fs");
const path = require("path");
const repo = path.join(__dirname, "..", "..");

function msgs(doc) {
    return doc.msgs.map((rec) => ({
        clientId: `client-${rec[0]}`, sequenceNumber: rec[1], referenceSequenceNumber: rec[2],
        minimumSequenceNumber: rec[3], contents: rec[4], type: rec.length > 5 ? rec[5] : "op",
    }));
}
const nul = (v) => (v === undefined ? null : v);
const und = (v) => (v === null ? undefined : v);

const docs = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const { GpuMergeTreeBatch } = require(path.join(repo, "fluidframework_amd", "js"));
const batch = new GpuMergeTreeBatch(docs.length, { segCapacity: 8192, textCapacity: 1 << 17 });
batch.loadInitialText(docs.map((d) => d.seed_text));
const clients = docs.map((d, i) => {
    const c = batch.client(i);
    c.startOrUpdateCollaboration("observer");
    return c;
});
docs.forEach((d, i) => { for (const m of msgs(d)) { clients[i].applyMsg(m); } });
batch.flush();

const out = docs.map((d, i) => {
    const c = clients[i];
    const mt = c.mergeTree;
    const o = { walks: [], args: { checked: 0, ok: 0 }, clones: [], texts: [], stops: [], throws: [] };
    d.views.forEach((v) => {
        const refSeq = v.refSeq === null ? c.getCurrentSeq() : v.refSeq;
        const per = [];
        v.walks.forEach(([start, end], k) => {
            const visits = [], accum = { k };
            mt.mapRange({ leaf: (seg, pos, r, cl, s, e, acc) => {
                o.args.checked++;
                if (r === refSeq && cl === v.client && acc === accum) { o.args.ok++; }
                visits.push([pos, s, e, seg.cachedLength, seg.seq, seg.clientId, nul(seg.text), nul(seg.refType)]);
                return true;
            } }, refSeq, v.client, accum, und(start), und(end));
            per.push(visits);
            if (visits.length > 2 && k % 5 === 0) {
                let n = 0;
                mt.mapRange({ leaf: () => { n++; return n < 2; } }, refSeq, v.client, undefined, und(start), und(end));
                o.stops.push([2, n, visits.length]);
            }
        });
        o.walks.push(per);
        const [s0, e0] = v.walks[0];
        const cl = mt.cloneSegments(refSeq, v.client, s0 === null ? undefined : s0, und(e0));
        const seen = new Set();
        mt.mapRange({ leaf: (seg) => { seen.add(seg); return true; } }, refSeq, v.client, undefined, und(s0), und(e0));
        o.clones.push([cl.map((s) => [s.cachedLength, nul(s.text)]), cl.every((s) => !seen.has(s))]);
        o.texts.push(v.texts.map(([k, ph]) => c.getTextInView(refSeq, v.client, ph, und(v.walks[k][0]), und(v.walks[k][1]))));
    });
    const v = d.views[d.views.length - 1];
    const tries = [["pre", () => mt.mapRange({ leaf: () => true, pre: () => true }, v.refSeq, v.client)],
        ["post", () => mt.mapRange({ leaf: () => true, post: () => true }, v.refSeq, v.client)],
        ["shift", () => mt.mapRange({ leaf: () => true, shift: () => true }, v.refSeq, v.client)],
        ["contains", () => mt.mapRange({ leaf: () => true, contains: () => true }, v.refSeq, v.client)],
        ["splitRange", () => mt.mapRange({ leaf: () => true }, v.refSeq, v.client, undefined, 0, 1, true)],
        ["star", () => c.getTextInView(v.refSeq, v.client, "*")]];
    for (const [name, f] of tries) {
        try { f(); o.throws.push([name, null]); } catch (e) { o.throws.push([name, e.message]); }
    }
    return o;
});
process.stdout.write(JSON.stringify({ docs: out }));
