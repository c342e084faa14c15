"use strict";
// Test driver for the Node facade's bulk / ranged text calls (fluidframework_amd/js).  Usage:
//   node tests/js/bulk_text_tool.js <fixture.json.gz> <ranges.json>
// ranges.json: per document a list of [start, end] (null: omitted).  Replays the fixture
// through GpuMergeTreeBatch and prints JSON {texts, docs: [{ranges, placeholders, helper,
// whole, foreign}]}: batch.getTexts(); per document client.getText(s, e) and
// client.getTextRangeWithPlaceholders(s, e) of every range, createTextHelper().getText(
// currentSeq, localId, " "), the argument-free getText() / getTextWithPlaceholders(), and the
// messages thrown for a foreign (refSeq, clientId) and a two-unit placeholder.
// The fixtures were produced by the reference itself (tests/golden/make_golden.py).
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
const thrown = (f) => { try { f(); return null; } catch (e) { return e.message; } };
const u = (v) => (v === null ? undefined : v);

const [file, rangesFile] = process.argv.slice(2);
const fx = JSON.parse(zlib.gunzipSync(fs.readFileSync(file)).toString("utf8"));
const ranges = JSON.parse(fs.readFileSync(rangesFile, "utf8"));
const { GpuMergeTreeBatch } = require(path.join(repo, "fluidframework_amd", "js"));
const batch = new GpuMergeTreeBatch(fx.docs.length, { segCapacity: 4096, textCapacity: 1 << 17 });
batch.loadInitialText(fx.docs.map((d) => d.seed_text));
const views = fx.docs.map((d, i) => {
    const c = batch.client(i);
    c.startOrUpdateCollaboration("observer");
    for (const m of msgs(d)) { c.applyMsg(m); }
    return c;
});
const texts = batch.getTexts();
const some = [fx.docs.length - 1, 0, 0];
const docs = views.map((c, i) => {
    const helper = c.createTextHelper();
    const seq = c.getCurrentSeq(), id = c.getClientId();
    return {
        ranges: ranges[i].map(([s, e]) => c.getText(u(s), u(e))),
        placeholders: ranges[i].map(([s, e]) => c.getTextRangeWithPlaceholders(u(s), u(e))),
        helper: helper.getText(seq, id, " "),
        helperRange: ranges[i].map(([s, e]) => helper.getText(seq, id, "", u(s), u(e))),
        whole: c.getText(),
        wholePlaceholders: c.getTextWithPlaceholders(),
        helperNoArgs: helper.getText(),
        foreign: [thrown(() => helper.getText(seq - 1, id, "")), thrown(() => helper.getText(seq, id + 1, ""))],
        longPlaceholder: thrown(() => helper.getText(seq, id, "ab")),
    };
});
process.stdout.write(JSON.stringify({ texts, some: batch.getTexts(some), docs }));
