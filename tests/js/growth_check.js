"use strict";
// Test driver for documents that grow, through the Node host: replays sequenced message lists,
// one ClientGroup document per list and one message per flush, on an engine of tiny capacities
// with ClientGroup's autogrow option, and prints what tests/test_growth.py compares with the
// oracle; then the explicit calls (resizeDocs / docCaps / docOccupancy) and an unarmed group
// on the same capacities, whose first document must overflow.
// usage: node growth_check.js IN.json OUT.json
const fs = require("fs");
const path = require("path");
const mt = require(path.join(__dirname, "..", "..", "fluidframework_amd", "js"));

const [inPath, outPath] = process.argv.slice(2);
const spec = JSON.parse(fs.readFileSync(inPath, "utf8"));
const n = spec.docs.length;
const eng = new mt.Engine(n, spec.limits);
const group = new mt.ClientGroup(eng, { autogrow: true });
const clients = spec.docs.map(() => {
    const c = group.newClient({ newMergeTreeSnapshotFormat: true });
    c.startOrUpdateCollaboration("observer");
    return c;
});
const len = Math.max(...spec.docs.map((m) => m.length));
for (let i = 0; i < len; i++) {
    spec.docs.forEach((msgs, d) => { if (i < msgs.length) clients[d].applyMsg(msgs[i]); });
    group.flush();
}
const out = { texts: clients.map((c) => c.getText()) };
const snaps = eng.snapshot(clients.map((c) => c.docId), clients.map((c) => c.minSeq), clients.map((c) => c.getCurrentSeq()), false);
out.digests = snaps.map((s) => s.digest.toString(16));
out.relocations = eng.growStats().relocations;
out.occupancy = eng.docOccupancy([0])[0];
eng.resizeDocs([0], { rowsPerDoc: 4096 });
out.capsAfterResize = eng.docCaps([0])[0];
out.textAfterResize = clients[0].getText();
eng.close();

const eng2 = new mt.Engine(1, spec.limits);
const c2 = new mt.ClientGroup(eng2).newClient({ newMergeTreeSnapshotFormat: true });
c2.startOrUpdateCollaboration("observer");
for (const m of spec.docs[0]) c2.applyMsg(m);
try { c2.group.flush(); } catch (e) { out.unarmedError = String(e); }
out.unarmedStatus = eng2.status([0])[0];
eng2.close();
fs.writeFileSync(outPath, JSON.stringify(out));
