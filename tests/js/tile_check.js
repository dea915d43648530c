"use strict";
// Test driver for tile search through the Node host: each case is a list of sequenced messages
// replayed on its own ClientGroup document, then a list of [startPos | null, label, preceding]
// findTile calls (null: an undefined startPos).  Prints per call {pos, refType, removedSeq} or
// null (undefined), or {error} when findTile throws; per case also the tile index of "EOP".
// usage: node tile_check.js IN.json OUT.json
const fs = require("fs");
const path = require("path");
const mt = require(path.join(__dirname, "..", "..", "fluidframework_amd", "js"));

const [inPath, outPath] = process.argv.slice(2);
const spec = JSON.parse(fs.readFileSync(inPath, "utf8"));
const eng = new mt.Engine(spec.cases.length, spec.limits);
const group = new mt.ClientGroup(eng);
const out = spec.cases.map((cs) => {
    const c = group.newClient();
    c.startOrUpdateCollaboration("observer");
    for (const m of cs.msgs) c.applyMsg(m);
    const calls = cs.calls.map(([pos, label, preceding]) => {
        try {
            const r = preceding === null ? c.findTile(pos === null ? undefined : pos, label)
                : c.findTile(pos === null ? undefined : pos, label, preceding);
            if (r === undefined) return null;
            return { pos: r.pos, refType: r.tile.refType, removedSeq: r.tile.removedSeq === undefined ? null : r.tile.removedSeq,
                labels: r.tile.properties.referenceTileLabels, json: r.tile.toJSONObject() };
        } catch (e) { return { error: String(e) }; }
    });
    const { recs, off } = eng.tileIndex([c.docId], "EOP");
    const index = [];
    for (let k = off[0]; k < off[1]; k++) index.push([recs[8 * k], recs[8 * k + 1]]);
    return { length: c.getLength(), calls, index };
});
eng.close();
fs.writeFileSync(outPath, JSON.stringify(out));
