// TEST INFRASTRUCTURE ONLY: drives the *transpiled reference* (oracle/_ref, built by
// oracle/build_ref.py) as the observer replica, the way tests/golden/walk_harness.mjs does, and
// records what MergeTree.mapRange({leaf}, refSeq, clientId, accum, start, end)
// (MT/mergeTree.ts:2830-2840 -> nodeMap, :2936-2998) hands its leaf action in sampled (refSeq,
// client) views, and what createTextHelper().getText(refSeq, clientId, placeholder, start, end)
// (MT/textSegment.ts:153-171) answers.  Run by tests/golden/make_view_walk.py.
// Usage: node tests/golden/view_walk_harness.mjs <logs.json> <out.json>
//   logs: {docs: [{doc, seed_text, msgs, checkpoints, writers, whole, seed}]}
//     writers: remote writers sampled per checkpoint; whole: 1 when whole-document queries are
//     asked in every view (0: one whole walk in the first remote view, short half-open ones in all); seed: of the random draws
// Per document and checkpoint (a message count):
//   n, minSeq, currentSeq
//   segs    [[cachedLength, seq, short client, removedSeq | null, removedClient | null,
//             removedClientOverlap ([]: none), refType | null (text), properties | null, text | null]]
//   levels  child counts of every tree level, bottom-up (levels[0]: rows per leaf block)
//   views   [{refSeq | null (the observer), client, stale 0|1, N (getLength), L (the leaves'
//             nodeLength sum), walks: [[start | null, end | null, [[row, pos, start, end] per visit]]],
//             texts: [[walk index, placeholder, text]]}]
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

// a small deterministic generator (the fixture must regenerate bit-identically)
function rng(seed) {
    let s = seed >>> 0;
    return (n) => {
        s = (Math.imul(s, 1664525) + 1013904223) >>> 0;
        return Math.floor((s / 4294967296) * n);
    };
}

// every step-th element of a list, the first and the last always
function sample(list, step) {
    return list.filter((_, i) => i % step === 0 || i === list.length - 1);
}

function checkpoint(c, n, log, latest, order, rand) {
    const mt = c.mergeTree;
    const minSeq = mt.collabWindow.minSeq;
    const currentSeq = mt.collabWindow.currentSeq;
    const rowOf = new Map();
    const segList = [];
    const segs = [];
    const inOverlap = new Map();      // short client -> rows whose overlap list holds it
    mt.walkAllSegments(mt.root, (seg) => {
        rowOf.set(seg, segs.length);
        segList.push(seg);
        const marker = Marker.is(seg);
        const ovl = seg.removedClientOverlap ? [...seg.removedClientOverlap] : [];
        for (const o of ovl) { inOverlap.set(o, (inOverlap.get(o) || 0) + 1); }
        segs.push([seg.cachedLength, seg.seq, seg.clientId,
            seg.removedSeq === undefined ? null : seg.removedSeq,
            seg.removedSeq === undefined ? null : seg.removedClientId, ovl,
            marker ? seg.refType : null,
            seg.properties !== undefined ? JSON.parse(JSON.stringify(seg.properties)) : null,
            marker ? null : seg.text]);
        return true;
    });
    // child counts per level, bottom-up, each level in document order; the level-1 nodes' first rows
    const levels = [];
    const pageRow = [];
    let rowsSeen = 0;
    const height = (block) => {
        if (block.childCount === 0 || block.children[0].isLeaf()) {
            (levels[0] = levels[0] || []).push(block.childCount);
            rowsSeen += block.childCount;
            return 0;
        }
        let h = -1;
        const level1 = block.children[0].childCount === 0 || block.children[0].children[0].isLeaf();
        if (level1) { pageRow.push(rowsSeen); }
        for (let i = 0; i < block.childCount; i++) {
            const hc = height(block.children[i]);
            if (h >= 0 && hc !== h) { throw new Error("uneven tree"); }
            h = hc;
        }
        (levels[h + 1] = levels[h + 1] || []).push(block.childCount);
        return h + 1;
    };
    height(mt.root);
    if (pageRow.length === 0) { pageRow.push(0); }

    // the views: the observer, then per sampled writer its latest refSeq, currentSeq, minSeq, the
    // one below its latest (stale) and two drawn at random
    const views = [{ refSeq: null, client: 0, stale: 0 }];
    const byOverlap = [...inOverlap.entries()].sort((a, b) => b[1] - a[1] || a[0] - b[0]).map((e) => e[0]);
    const writers = [];
    for (const k of byOverlap.slice(0, Math.ceil(log.writers / 2)).concat([...order].reverse())) {
        if (!writers.includes(k) && writers.length < log.writers && latest.has(k)) { writers.push(k); }
    }
    for (const k of writers) {
        const last = latest.get(k);
        const want = [last, currentSeq, minSeq, last - 1, minSeq + rand(currentSeq - minSeq + 1),
            minSeq + rand(currentSeq - minSeq + 1)];
        const seen = new Set();
        for (const r of want) {
            if (r < minSeq || r > currentSeq || seen.has(r)) { continue; }
            seen.add(r);
            views.push({ refSeq: r, client: k, stale: r < last ? 1 : 0 });
        }
    }
    const helper = c.createTextHelper();
    let remoteSeen = 0;
    for (const v of views) {
        const refSeq = v.refSeq === null ? currentSeq : v.refSeq;
        const clientId = v.refSeq === null ? mt.collabWindow.clientId : v.client;
        const lens = segList.map((s) => mt.nodeLength(s, refSeq, clientId));
        const N = mt.getLength(refSeq, clientId);
        const L = lens.reduce((a, b) => a + b, 0);
        v.N = N;
        v.L = L;
        const bounds = [];
        const inside = [];
        const prefix = [];
        let pos = 0;
        lens.forEach((len) => {
            prefix.push(pos);
            if (len > 0) {
                bounds.push(pos);
                if (len >= 4) { inside.push(pos + (len >> 1)); }
                pos += len;
            }
        });
        const whole = log.whole || (v.refSeq !== null && remoteSeen === 0);
        if (v.refSeq !== null) { remoteSeen++; }
        const queries = [];
        if (log.whole) {   // (all four in every third view, two in the others)
            queries.push([undefined, undefined]);
            if (views.indexOf(v) % 3 === 0) { queries.push([0, N], [undefined, Math.max(N >> 1, 0)]); }
            queries.push([N - (N >> 2), undefined]);
        } else {
            if (whole) { queries.push([undefined, undefined]); }
            queries.push([Math.max(N - 40, 0), undefined], [undefined, 30]);
        }
        const nb = log.whole ? 4 : 3;
        for (const p of sample(bounds, Math.max(1, Math.ceil(bounds.length / nb)))) {
            queries.push([p, p], [p, p + 1], [p - 1, p + 1]);
        }
        for (const p of sample(inside, Math.max(1, Math.ceil(inside.length / nb)))) {
            queries.push([p, p], [p + 1, p - 1]);
        }
        queries.push([N - 1, N + 5], [N, N], [N + 1, N + 3]);
        // ranges inside one level-1 node, across two, and starting beyond the 64th
        const nPages = pageRow.length;
        const asked = sample([...Array(nPages).keys()], Math.max(1, Math.ceil(nPages / 4)));
        if (nPages > 66) { asked.push(64, 65, nPages - 2); }
        const at = (j) => (j < nPages ? (pageRow[j] < prefix.length ? prefix[pageRow[j]] : L) : L);
        for (const j of asked) {
            const lo = at(j);
            const hi = at(j + 1);
            if (hi - lo >= 3) { queries.push([lo + 1, hi - 1]); }
            if (j + 1 < nPages && hi - lo >= 2 && at(j + 2) - hi >= 2) { queries.push([hi - 2, hi + 2]); }
        }
        v.walks = [];
        v.texts = [];
        for (const [start, end] of queries) {
            if (start !== undefined && start < 0) { continue; }
            const visits = [];
            mt.mapRange({
                leaf: (seg, p, r, cl, s, e, accum) => {
                    if (!rowOf.has(seg)) { throw new Error("mapRange handed out a segment outside the tree"); }
                    if (accum !== visits || r !== refSeq || cl !== clientId) { throw new Error("arguments not passed through"); }
                    visits.push([rowOf.get(seg), p, s, e]);
                    return true;
                },
            }, refSeq, clientId, visits, start, end);
            const i = v.walks.length;
            v.walks.push([start === undefined ? null : start, end === undefined ? null : end, visits]);
            // the texts: clipped ranges (the reversed ones among them), a few whole ones
            const clipped = start !== undefined && end !== undefined && Math.abs(end - start) <= 300;
            if ((clipped && i % 3 === 0) || (whole && i < 2 && N <= 4000)) {
                const ph = (i >> 1) % 2 === 0 ? "" : " ";
                v.texts.push([i, ph, helper.getText(refSeq, clientId, ph, start, end)]);
            }
        }
    }
    return { n, minSeq, currentSeq, segs, levels, views };
}

function walkDoc(log) {
    const c = new Client(segmentFromSpec, logger);
    if (log.seed_text.length > 0) { c.insertSegmentLocal(0, TextSegment.make(log.seed_text)); }
    c.startOrUpdateCollaboration("observer");
    const cseq = {};
    const out = [];
    const latest = new Map();   // short client -> the refSeq of its latest message
    const order = [];           // short clients, by their latest message (oldest first)
    const rand = rng(log.seed);
    let next = 0;
    log.msgs.forEach(([k, t, r, msn, op, type], i) => {
        if (next >= log.checkpoints.length) { return; }
        cseq[k] = (cseq[k] || 0) + 1;
        const msg = makeMsg(k, t, r, msn, cseq[k], JSON.parse(JSON.stringify(op)));
        if (type) { msg.type = type; }
        c.applyMsg(msg);
        const short = c.getOrAddShortClientId(`client-${k}`);
        latest.set(short, r);
        const at = order.indexOf(short);
        if (at >= 0) { order.splice(at, 1); }
        order.push(short);
        if (log.checkpoints[next] === i + 1) {
            out.push(checkpoint(c, i + 1, log, latest, order, rand));
            next++;
        }
    });
    return { doc: log.doc, checkpoints: out };
}

const [inp, outp] = process.argv.slice(2);
const logs = JSON.parse(fs.readFileSync(inp, "utf8"));
fs.writeFileSync(outp, JSON.stringify({ docs: logs.docs.map((d) => walkDoc(d)) }));
