"use strict";
// Test driver for text ranges through the Node host: each case is a list of sequenced messages
// replayed on its own document (a MergeTreeClient, or a SequenceChannel when `channel` is set),
// then a list of calls (null stands for undefined):
//   ["helper", refSeq, longClientId | null, placeholder | null, start, end]  createTextHelper().getText
//   ["getText", start, end]                       MergeTreeClient / SequenceChannel getText
//   ["withPlaceholders"] | ["rangeWithPlaceholders", start, end] | ["rangeWithMarkers", start, end]
//   ["raw", [start...], [end...], placeholder]    Engine.getTextRange of this document, local view
// Prints per call the string (or the list of strings), or {error, name} when the call throws.
// usage: node text_check.js IN.json OUT.json
const fs = require("fs");
const path = require("path");
const mt = require(path.join(__dirname, "..", "..", "fluidframework_amd", "js"));

const [inPath, outPath] = process.argv.slice(2);
const spec = JSON.parse(fs.readFileSync(inPath, "utf8"));
const eng = new mt.Engine(spec.cases.length, spec.limits);
const group = new mt.ClientGroup(eng);
const u = (v) => (v === null ? undefined : v);
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
            if (kind === "helper") {
                const id = a[1] === null ? 0 : c.getShortClientId(a[1]);
                const h = c.createTextHelper();
                return a[2] === null ? h.getText(a[0], id) : h.getText(a[0], id, a[2], u(a[3]), u(a[4]));
            }
            if (kind === "getText") return (ch || c).getText(u(a[0]), u(a[1]));
            if (kind === "withPlaceholders") return ch.getTextWithPlaceholders();
            if (kind === "rangeWithPlaceholders") return ch.getTextRangeWithPlaceholders(u(a[0]), u(a[1]));
            if (kind === "rangeWithMarkers") return ch.getTextRangeWithMarkers(u(a[0]), u(a[1]));
            if (kind === "raw") {
                c.group.flush();
                return eng.getTextRange(a[0].map(() => c.docId), a[0].map(u), a[1].map(u), undefined, undefined, a[2]);
            }
            throw new Error(`unknown call ${kind}`);
        } catch (e) { return { error: String(e), name: e.name }; }
    });
    return { length: c.getLength(), calls };
});
eng.close();
fs.writeFileSync(outPath, JSON.stringify(out));
