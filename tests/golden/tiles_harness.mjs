// TEST INFRASTRUCTURE ONLY: drives the *transpiled reference* (oracle/_ref, built by
// oracle/build_ref.py) as the observer replica, the way oracle/ref_harness.mjs does, and records
// what SharedString.findTile / getMarkerFromId answer (SEQ/sharedString.ts:214, :242 are
// one-liners onto Client.findTile, MT/client.ts:1075, and MergeTree.getMarkerFromId,
// MT/mergeTree.ts:1965).  Run by tests/golden/make_tiles.py.
// Usage: node tests/golden/tiles_harness.mjs <logs.json> <out.json>
//   logs: {labels: [...], docs: [{doc, seed_text, msgs, checkpoints, sample}]} (tests/tile_streams.py)
// Per document and checkpoint (a message count):
//   n, length
//   segs   [[cachedLength, removed 0|1, refType | null (text), properties | null (text rows: null)]]
//   leaves rows per leaf block; pages: rows per level-1 node (a root of leaves: one page)
//   tiles  [[pos | null (undefined), label index, preceding 0|1, row | -1, pos of the tile | -1]]
//   ids    [[id, row | -1 (not among the tree's leaves), still its parent's child 0|1, found 0|1]]
//          for every markerId inserted so far
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

function checkpoint(c, n, labels, ids, sample) {
    const mt = c.mergeTree;
    const rowOf = new Map();
    const segs = [];
    const tilePos = [];
    let tileCount = 0;
    mt.walkAllSegments(mt.root, (seg) => {
        rowOf.set(seg, segs.length);
        const marker = Marker.is(seg);
        const removed = seg.removedSeq === undefined ? 0 : 1;
        segs.push([seg.cachedLength, removed, marker ? seg.refType : null,
            marker && seg.properties !== undefined ? JSON.parse(JSON.stringify(seg.properties)) : null]);
        if (marker && !removed && (seg.refType & 1)) {
            if (tileCount++ % sample === 0) { tilePos.push(c.getPosition(seg)); }
        }
        return true;
    });
    const leaves = [];
    const pages = [];
    const walk = (block, top) => {
        if (block.childCount === 0 || block.children[0].isLeaf()) {
            leaves.push(block.childCount);
            if (top) { pages.push(block.childCount); } else { pages[pages.length - 1] += block.childCount; }
            return;
        }
        const level1 = block.children[0].childCount === 0 || block.children[0].children[0].isLeaf();
        if (level1) { pages.push(0); }
        for (let i = 0; i < block.childCount; i++) { walk(block.children[i], false); }
    };
    walk(mt.root, true);
    const length = c.getLength();
    const posSet = new Set([0, length - 1, length, length + 1]);
    for (const p of tilePos) { posSet.add(p - 1); posSet.add(p); posSet.add(p + 1); }
    const positions = [...posSet].filter((p) => p >= 0).sort((a, b) => a - b);
    positions.push(undefined);
    const tiles = [];
    for (const pos of positions) {
        for (let l = 0; l < labels.length; l++) {
            for (const preceding of [true, false]) {
                const r = c.findTile(pos, labels[l], preceding);
                const q = [pos === undefined ? null : pos, l, preceding ? 1 : 0];
                if (r === undefined) {
                    q.push(-1, -1);
                } else {
                    if (!rowOf.has(r.tile)) { throw new Error("findTile returned a segment outside the tree"); }
                    q.push(rowOf.get(r.tile), r.pos);
                }
                tiles.push(q);
            }
        }
    }
    const byId = ids.map((id) => {
        const seg = mt.getMarkerFromId(id);
        if (seg === undefined) { return [id, -1, 0, 0]; }
        const p = seg.parent;
        const linked = p !== undefined && p.children.slice(0, p.childCount).includes(seg);
        return [id, rowOf.has(seg) ? rowOf.get(seg) : -1, linked ? 1 : 0, 1];
    });
    return { n, length, segs, leaves, pages, tiles, ids: byId };
}

function tilesDoc(log, labels) {
    const c = new Client(segmentFromSpec, logger);
    if (log.seed_text.length > 0) { c.insertSegmentLocal(0, TextSegment.make(log.seed_text)); }
    c.startOrUpdateCollaboration("observer");
    const cseq = {};
    const ids = [];
    const out = [];
    let next = 0;
    log.msgs.forEach(([k, t, r, msn, op, type], i) => {
        cseq[k] = (cseq[k] || 0) + 1;
        const msg = makeMsg(k, t, r, msn, cseq[k], JSON.parse(JSON.stringify(op)));
        if (type) { msg.type = type; }
        c.applyMsg(msg);
        if (op && op.type === 0 && op.seg.marker && op.seg.props && op.seg.props.markerId !== undefined) {
            ids.push(op.seg.props.markerId);
        }
        if (next < log.checkpoints.length && log.checkpoints[next] === i + 1) {
            out.push(checkpoint(c, i + 1, labels, ids, log.sample || 1));
            next++;
        }
    });
    return { doc: log.doc, checkpoints: out };
}

const [inp, outp] = process.argv.slice(2);
const logs = JSON.parse(fs.readFileSync(inp, "utf8"));
fs.writeFileSync(outp, JSON.stringify({ docs: logs.docs.map((d) => tilesDoc(d, logs.labels)) }));
