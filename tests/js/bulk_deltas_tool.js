"use strict";
// Test driver for the Node facade's bulk delta-log drain (tests/test_js_bulk_deltas.py).  Usage:
//   node tests/js/bulk_deltas_tool.js slices <fixture.json.gz>
//       -> {equal: [bool per doc], off, words, rowOff, rows, flags, sub: {...}} : native
//          getDeltaLogs against native getDeltaLog on one applied batch
//   node tests/js/bulk_deltas_tool.js views <fixture.json.gz> <ranges 0|1> <first flush messages>
//       -> {calls: {doc: [...]}, ranges: [per flush {rowOff, rows, flags} | null], error}: the first 8
//          documents, views on documents 1, 4 and 6 only, two flushes
const fs = require("fs");
const zlib = require("zlib");
const path = require("path");
const repo = path.join(__dirname, "..", "..");
const { GpuMergeTreeBatch, native } = require(path.join(repo, "fluidframework_amd", "js"));

function msgs(doc) {
    return doc.msgs.map((rec) => ({
        clientId: `client-${rec[0]}`, sequenceNumber: rec[1], referenceSequenceNumber: rec[2],
        minimumSequenceNumber: rec[3], contents: rec[4], type: rec.length > 5 ? rec[5] : "op",
    }));
}
const [mode, file, ...extra] = process.argv.slice(2);
const fx = JSON.parse(zlib.gunzipSync(fs.readFileSync(file)).toString("utf8"));
const arr = (a) => Array.from(a);
const OPTS = { segCapacity: 8192, textCapacity: 1 << 17, deltaLogCapacity: 1 << 18, deltaLogMode: 0 };

if (mode === "slices") {
    const batch = new GpuMergeTreeBatch(fx.docs.length, OPTS);
    batch.loadInitialText(fx.docs.map((d) => d.seed_text));
    fx.docs.forEach((d, i) => { for (const m of msgs(d)) { batch.pending[i].push(m); batch.queued++; } });
    // (applied below the facade, whose flush drains and resets the logs)
    const a = batch._encodePending();
    native.applyOps(batch.h, a.docOff, a.ops, a.text, a.props);
    const singles = fx.docs.map((d, i) => native.getDeltaLog(batch.h, i));
    const same = (x, y) => x.length === y.length && x.every((v, k) => v === y[k]);
    const r = native.getDeltaLogs(batch.h, null, null, true);
    const equal = singles.map((s, i) => same(s, r.words.subarray(r.off[i], r.off[i + 1])));
    // a subset, reversed, one record in
    const docs = Uint32Array.from([5, 2, 2, 0]);
    const firstRecord = (log) => {
        let i = 3;
        for (let k = 0; k < log[2]; k++) {
            i += 2;
            if (log[1] === 2) { i += 1 + 2 * Math.max(log[i], 0); }
        }
        return i;
    };
    const from = Int32Array.from(docs, (d) => firstRecord(singles[d]));
    const s = native.getDeltaLogs(batch.h, docs, from);
    const subEqual = arr(docs).map((d, q) => same(singles[d].subarray(from[q]), s.words.subarray(s.off[q], s.off[q + 1])));
    native.deltaLogResetDocs(batch.h, Uint32Array.from([1, 3]));
    const after = native.getDeltaLogs(batch.h, null, null);
    process.stdout.write(JSON.stringify({
        equal, off: arr(r.off), words: arr(r.words), rowOff: arr(r.rowOff), rows: arr(r.rows), flags: arr(r.flags),
        subEqual, subFlags: arr(s.flags), noRows: s.rows === undefined && s.rowOff === undefined,
        afterReset: arr(after.off).map((o, i, all) => (i ? o - all[i - 1] : 0)).slice(1),
    }));
} else if (mode === "views") {
    const ranges = extra[0] === "1", first = parseInt(extra[1], 10);
    const docsFx = fx.docs.slice(0, 8);
    const batch = new GpuMergeTreeBatch(8, Object.assign({ deltaRanges: ranges ? 1 : 0 }, OPTS));
    batch.loadInitialText(docsFx.map((d) => d.seed_text));
    const calls = {};
    const views = {};
    for (const i of [1, 4, 6]) {
        const c = batch.client(i);
        c.startOrUpdateCollaboration("observer");
        calls[i] = [];
        c.mergeTreeDeltaCallback = (opArgs, args) => {
            calls[i].push([opArgs.sequencedMessage.sequenceNumber, args.operation,
                args.deltaSegments.map((x) => (x.propertyDeltas !== undefined ? [x.position, x.segment.cachedLength, x.propertyDeltas]
                    : [x.position, x.segment.cachedLength]))]);
        };
        views[i] = c;
    }
    const all = docsFx.map((d) => msgs(d));
    const out = [];
    let error = null;
    try {
        for (const [lo, hi] of [[0, first], [first, Infinity]]) {
            all.forEach((m, i) => {
                for (const x of m.slice(lo, hi)) {
                    if (views[i]) { views[i].applyMsg(x); } else { batch.pending[i].push(x); batch.queued++; }
                }
            });
            batch.flush();
            const r = ranges ? batch.getDeltaRanges() : null;
            out.push(r ? { rowOff: arr(r.rowOff), rows: arr(r.rows), flags: arr(r.flags) } : null);
        }
    } catch (e) {
        error = e.message;
    }
    process.stdout.write(JSON.stringify({ calls, ranges: out, error }));
} else {
    throw new Error(`unknown mode ${mode}`);
}
