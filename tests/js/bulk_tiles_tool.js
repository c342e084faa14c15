"use strict";
// Test driver for the Node facade's marker queries (fluidframework_amd/js).  Usage:
//   node tests/js/bulk_tiles_tool.js <ref_tiles fixture.json.gz> <flushEvery (0: one flush)>
// Replays the fixture through GpuClients whose delta callbacks keep, per markerId, the segment
// object the insert event carried, then prints JSON per document for its final checkpoint:
//   tiles  [[row, pos] | null] of one batch.findTiles call for every findTile query
//   ids    [row | null] of one batch.getMarkersFromIds call for every id
//   client {checked, posEqual, sameObject}: GpuClient.findTile on a sample of the queries (every
//          one of a small document) -- pos equal to the bulk answer, tile the event's object
//   byId   {checked, sameObject, gone}: GpuClient.getMarkerFromId of every id -- the event's
//          object, undefined exactly where the bulk answer is
// The fixture was produced by the reference itself (tests/golden/make_tiles.py).
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

const [file, every] = process.argv.slice(2);
const flushEvery = parseInt(every, 10);
const fx = JSON.parse(zlib.gunzipSync(fs.readFileSync(file)).toString("utf8"));
const { GpuMergeTreeBatch } = require(path.join(repo, "fluidframework_amd", "js"));
const batch = new GpuMergeTreeBatch(fx.docs.length, { segCapacity: 8192, textCapacity: 1 << 17, deltaLogCapacity: 1 << 20 });
batch.loadInitialText(fx.docs.map((d) => d.seed_text));
const carried = fx.docs.map(() => new Map());   // per document: markerId -> the insert event's segment
const views = fx.docs.map((d, i) => {
    const c = batch.client(i);
    c.startOrUpdateCollaboration("observer");
    c.mergeTreeDeltaCallback = (opArgs, args) => {
        if (args.operation !== 0) { return; }
        for (const x of args.deltaSegments) {
            const p = x.segment.properties;
            if (x.segment.type === "Marker" && p && p.markerId !== undefined) { carried[i].set(p.markerId, x.segment); }
        }
    };
    return c;
});
const all = fx.docs.map(msgs);
const longest = Math.max(...all.map((m) => m.length));
for (let at = 0; at < longest; at += flushEvery || longest) {
    all.forEach((m, i) => { for (const x of m.slice(at, at + (flushEvery || longest))) { views[i].applyMsg(x); } });
    batch.flush();
}
const last = fx.docs.map((d) => d.checkpoints[d.checkpoints.length - 1]);
const tq = [], iq = [];
last.forEach((cp, i) => {
    for (const [pos, lab, prec] of cp.tiles) {
        tq.push({ doc: i, pos: pos === null ? undefined : pos, label: fx.labels[lab], preceding: prec === 1 });
    }
    for (const [id] of cp.ids) { iq.push({ doc: i, id }); }
});
const tiles = batch.findTiles(tq);
const ids = batch.getMarkersFromIds(iq);
const out = fx.docs.map(() => ({ tiles: [], ids: [], client: { checked: 0, posEqual: 0, sameObject: 0 },
    byId: { checked: 0, sameObject: 0, gone: 0 } }));
tq.forEach((q, k) => {
    const o = out[q.doc], t = tiles[k];
    o.tiles.push(t === undefined ? null : [t.row, t.position]);
    if (last[q.doc].tiles.length > 200 && k % 7 !== 0) { return; }
    const r = views[q.doc].findTile(q.pos, q.label, q.preceding);
    o.client.checked++;
    if ((r === undefined) === (t === undefined) && (r === undefined || r.pos === t.position)) { o.client.posEqual++; }
    if (r === undefined) { o.client.sameObject++; return; }
    const id = r.tile.properties && r.tile.properties.markerId;
    // (a marker without an id was carried by no recorded event: it is a Marker of that refType)
    if (id !== undefined ? r.tile === carried[q.doc].get(id) : (r.tile.type === "Marker" && r.tile.refType === t.markerRefType)) {
        o.client.sameObject++;
    }
});
iq.forEach((q, k) => {
    const o = out[q.doc], t = ids[k];
    o.ids.push(t === undefined ? null : t.row);
    const seg = views[q.doc].getMarkerFromId(q.id);
    o.byId.checked++;
    if (seg === undefined) { if (t === undefined) { o.byId.gone++; o.byId.sameObject++; } return; }
    if (t !== undefined && seg === carried[q.doc].get(q.id) && seg.properties.markerId === q.id) { o.byId.sameObject++; }
});
process.stdout.write(JSON.stringify({ docs: out, never: [views[0].findTile(0, "never-seen"), views[0].getMarkerFromId("never-seen"),
    views[0].getMarkerFromId("")].map((x) => (x === undefined ? null : x)) }));
