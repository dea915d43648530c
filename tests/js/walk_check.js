"use strict";
// Test driver for segment walks through the Node host: each case is a list of sequenced messages
// replayed on its own document (a MergeTreeClient, or a SequenceChannel when `channel` is set),
// then a list of calls (null stands for undefined):
//   ["walk", start, end, accum, stopAt, ret]  walkSegments with a handler that returns true until
//       its stopAt-th call, where it returns ret ("undefined": nothing); per visit
//       [toJSONObject, pos, refSeq, clientId, start, end, accum, cachedLength, seq, removedSeq,
//       properties, getPosition]
//   ["split", start, end]                     walkSegments(..., splitRange = true)
//   ["raw", [start...], [end...], refSeq, longClientId | null, text]  Engine.walkSegments of this
//       document under one view: {off, recs: [[14 fields]...], texts, maps: [JSON texts], objs}
// Prints per call the result, or {error, name} when the call throws.
// usage: node walk_check.js IN.json OUT.json
const fs = require("fs");
const path = require("path");
const mt = require(path.join(__dirname, "..", "..", "fluidframework_amd", "js"));

const [inPath, outPath] = process.argv.slice(2);
const spec = JSON.parse(fs.readFileSync(inPath, "utf8"));
const eng = new mt.Engine(spec.cases.length, spec.limits);
const group = new mt.ClientGroup(eng);
const u = (v) => (v === null ? undefined : v);
const n = (v) => (v === undefined ? null : v);
const out = spec.cases.map((cs) => {
    let c, ch;
    if (cs.channel) {
        ch = new mt.SequenceChannel(group, { clientId: "observer", options: { newMergeTreeSnapshotFormat: true } });
        c = ch.client;
        for (const m of cs.msgs) ch.processCore(m, false);
    } else {
        c = group.newClient();
        c.startOrUpdateCollaboration("observer");
        for (const m of cs.msgs) c.applyMsg(m);
    }
    group.flush();                                  // the clients' short ids exist once their messages are packed
    const calls = cs.calls.map(([kind, ...a]) => {
        try {
            if (kind === "walk") {
                const seen = [];
                (ch || c).walkSegments((seg, pos, refSeq, clientId, start, end, accum) => {
                    seen.push([seg.toJSONObject(), pos, refSeq, clientId, start, end, n(accum), seg.cachedLength, seg.seq, n(seg.removedSeq),
                        n(seg.properties), c.getPosition(seg)]);
                    if (seen.length !== a[3]) return true;
                    return a[4] === "undefined" ? undefined : a[4];
                }, u(a[0]), u(a[1]), u(a[2]));
                return seen;
            }
            if (kind === "split") { (ch || c).walkSegments(() => true, u(a[0]), u(a[1]), undefined, true); return "walked"; }
            if (kind === "raw") {
                c.group.flush();
                const k = a[0].length;
                const local = a[3] === null;
                const w = eng.walkSegments(a[0].map(() => c.docId), a[0].map(u), a[1].map(u), a[0].map(() => (local ? -1 : a[2])),
                    a[0].map(() => (local ? -1 : c.getShortClientId(a[3]) - 1)), a[4]);
                if (!(w.recs instanceof Int32Array) || !(w.units instanceof Uint16Array) || w.off.length !== k + 1) throw new Error("not typed arrays");
                const recs = [], texts = [];
                for (let r = 0; r < w.off[k]; r++) {
                    const f = Array.from(w.recs.subarray(16 * r, 16 * r + 14));
                    recs.push(f);
                    texts.push(f[10] >= 0 || !a[4] ? null : String.fromCharCode.apply(null, w.units.subarray(w.recs[16 * r + 14], w.recs[16 * r + 14] + f[3])));
                }
                return { off: Array.from(w.off), recs, texts, maps: w.maps.json, objs: w.maps.json.map((_, m) => eng.walkMapObject(w.maps, m)) };
            }
            throw new Error(`unknown call ${kind}`);
        } catch (e) { return { error: String(e), name: e.name }; }
    });
    return { length: c.getLength(), calls };
});
eng.close();
fs.writeFileSync(outPath, JSON.stringify(out));
