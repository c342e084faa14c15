// TEST INFRASTRUCTURE ONLY: drives the *transpiled reference* (oracle/_ref, built by
// oracle/build_ref.py) as the observer replica, the way oracle/ref_harness.mjs does, and records
// what Client.walkSegments (MT/client.ts:276-285) hands its handler for a list of ranges, what
// createTextHelper().getTextAndMarkers (MT/textSegment.ts:127-152) answers for every label, and
// Client.getRangeExtentsOfPosition (MT/client.ts:1026-1043).  Run by tests/golden/make_walk.py.
// Usage: node tests/golden/walk_harness.mjs <logs.json> <out.json>
//   logs: {labels: [...], docs: [{doc, seed_text, msgs, checkpoints}]} (tests/walk_streams.py)
// Per document and checkpoint (a message count):
//   n, length
//   segs    [[cachedLength, removed 0|1, refType | null (text), properties | null (undefined),
//             text | null (marker), seq, short client]]
//   leaves  rows per leaf block; pages: rows per level-1 node (a root of leaves: one page)
//   walks   [[start | null (undefined), end | null, [[row, pos, start, end] per visit]]]
//   tam     per label: [parallelText, rows of parallelMarkers]
//   extents [[pos, posStart | null, posAfterEnd | null]]
import fs from "fs";
import * as MT from "../../oracle/_ref/mt/index.mjs";

const { Client, TextSegment, Marker } = MT;

function segmentFromSpec(spec) {           // SEQ/sequenceFactory.ts:31-37
    const t = TextSegment.fromJSONObject(spec);
    if (t) { return t; }
    const m = Marker.fromJSONObject(spec);
    if (m) { return m; }
    throw new Error("bad spec");
}
const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };

function makeMsg(k, seq, ref, msn, cseq, contents) {
    return {
        clientId: `client-${k}`, sequenceNumber: seq, referenceSequenceNumber: ref,
        minimumSequenceNumber: msn, clientSequenceNumber: cseq, type: "op", contents,
        timestamp: 0, term: 1, traces: [],
    };
}

// every step-th element of a list, the first and the last always
function sample(list, step) {
    return list.filter((_, i) => i % step === 0 || i === list.length - 1);
}

function checkpoint(c, n, labels) {
    const mt = c.mergeTree;
    const rowOf = new Map();
    const segs = [];
    const bounds = [];          // positions where a visible row starts
    const inside = [];          // points strictly inside visible rows of length >= 4
    let pos = 0;
    mt.walkAllSegments(mt.root, (seg) => {
        rowOf.set(seg, segs.length);
        const marker = Marker.is(seg);
        const removed = seg.removedSeq === undefined ? 0 : 1;
        segs.push([seg.cachedLength, removed, marker ? seg.refType : null,
            seg.properties !== undefined ? JSON.parse(JSON.stringify(seg.properties)) : null,
            marker ? null : seg.text, seg.seq, seg.clientId]);
        if (!removed && seg.cachedLength > 0) {
            bounds.push(pos);
            if (seg.cachedLength >= 4) { inside.push(pos + (seg.cachedLength >> 1)); }
            pos += seg.cachedLength;
        }
        return true;
    });
    const leaves = [];
    const pages = [];
    const pageStart = [];       // the position where each level-1 node starts
    let at = 0;
    const walk = (block, top) => {
        if (block.childCount === 0 || block.children[0].isLeaf()) {
            leaves.push(block.childCount);
            if (top) { pages.push(block.childCount); pageStart.push(0); } else { pages[pages.length - 1] += block.childCount; }
            for (let i = 0; i < block.childCount; i++) {
                const s = block.children[i];
                if (s.removedSeq === undefined) { at += s.cachedLength; }
            }
            return;
        }
        const level1 = block.children[0].childCount === 0 || block.children[0].children[0].isLeaf();
        if (level1) { pages.push(0); pageStart.push(at); }
        for (let i = 0; i < block.childCount; i++) { walk(block.children[i], false); }
    };
    walk(mt.root, true);
    const length = c.getLength();
    if (pos !== length || at !== length) { throw new Error("length mismatch"); }

    const queries = [[undefined, undefined], [0, length], [undefined, Math.max(length >> 1, 0)], [length >> 2, undefined]];
    for (const p of sample(bounds, Math.max(1, Math.ceil(bounds.length / 24)))) {
        queries.push([p, p], [p, p + 1], [p - 1, p + 1]);
    }
    for (const p of sample(inside, Math.max(1, Math.ceil(inside.length / 16)))) {
        queries.push([p, p], [p + 1, p - 1], [p + 2, p]);
    }
    queries.push([length - 1, length + 5], [length, length], [length + 1, length + 3], [0, 0], [0, 1]);
    // ranges inside one page, across two pages, and starting beyond the first 64 directory positions
    const nPages = pages.length;
    const pagesAsked = sample([...Array(nPages).keys()], Math.max(1, Math.ceil(nPages / 8)));
    if (nPages > 66) { pagesAsked.push(64, 65, 66, nPages - 2); }
    for (const j of pagesAsked) {
        const lo = pageStart[j];
        const hi = j + 1 < nPages ? pageStart[j + 1] : length;
        if (hi - lo >= 3) { queries.push([lo + 1, hi - 1]); }
        if (j + 1 < nPages) {
            const hi2 = j + 2 < nPages ? pageStart[j + 2] : length;
            if (hi - lo >= 2 && hi2 - hi >= 2) { queries.push([hi - 2, hi + 2], [lo + 1, hi2 - 1]); }
        }
    }
    const walks = [];
    for (const [start, end] of queries) {
        if (start !== undefined && start < 0) { continue; }
        const visits = [];
        c.walkSegments((seg, p, refSeq, clientId, s, e, accum) => {
            if (!rowOf.has(seg)) { throw new Error("walkSegments handed out a segment outside the tree"); }
            if (accum !== visits) { throw new Error("accum not passed through"); }
            visits.push([rowOf.get(seg), p, s, e]);
            return true;
        }, start, end, visits);
        walks.push([start === undefined ? null : start, end === undefined ? null : end, visits]);
    }
    const helper = c.createTextHelper();
    const tam = labels.map((label) => {
        const r = helper.getTextAndMarkers(c.getCurrentSeq(), c.getClientId(), label);
        return [r.parallelText, r.parallelMarkers.map((m) => {
            if (!rowOf.has(m)) { throw new Error("getTextAndMarkers returned a marker outside the tree"); }
            return rowOf.get(m);
        })];
    });
    const extentsAt = new Set([0, 1, length >> 1, length - 1, length, length + 1]);
    for (const p of sample(inside, Math.max(1, Math.ceil(inside.length / 4)))) { extentsAt.add(p); }
    const extents = [...extentsAt].filter((p) => p >= 0).sort((a, b) => a - b).map((p) => {
        const r = c.getRangeExtentsOfPosition(p);
        return [p, r.posStart === undefined ? null : r.posStart, r.posAfterEnd === undefined ? null : r.posAfterEnd];
    });
    return { n, length, segs, leaves, pages, walks, tam, extents };
}

function walkDoc(log, labels) {
    const c = new Client(segmentFromSpec, logger);
    if (log.seed_text.length > 0) { c.insertSegmentLocal(0, TextSegment.make(log.seed_text)); }
    c.startOrUpdateCollaboration("observer");
    const cseq = {};
    const out = [];
    let next = 0;
    log.msgs.forEach(([k, t, r, msn, op, type], i) => {
        cseq[k] = (cseq[k] || 0) + 1;
        const msg = makeMsg(k, t, r, msn, cseq[k], JSON.parse(JSON.stringify(op)));
        if (type) { msg.type = type; }
        c.applyMsg(msg);
        if (next < log.checkpoints.length && log.checkpoints[next] === i + 1) {
            out.push(checkpoint(c, i + 1, labels));
            next++;
        }
    });
    return { doc: log.doc, checkpoints: out };
}

const [inp, outp] = process.argv.slice(2);
const logs = JSON.parse(fs.readFileSync(inp, "utf8"));
fs.writeFileSync(outp, JSON.stringify({ docs: logs.docs.map((d) => walkDoc(d, logs.labels)) }));
