"""Diagnostic: how the zamboni's merge-run text moves (gatherText) are spread over scourLeaves
calls, on the host emulation built with -DMT_EVGATHER; the same generator and seeds as bench.py
on a subset of documents.  Not the product.

usage: python tools/event_stats_gather.py [config2] [docs=16] [residency=blk]
"""
import ctypes as C, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from fluidframework_amd.engine import Engine
from fluidframework_amd.batch import MtGenParams
import bench

AFTER = "gathers after a gather in their call"
# (slot, high half) of every counter, as mt_core.h lays them out (MT_EVG)
LAYOUT = {"scourLeaves calls": (0, 0), "calls with a gather": (0, 1), "gathers": (1, 0), AFTER: (1, 1),
          "64-unit chunks": (2, 0), "units": (3, 0), "calls that load a last unit (lastNL)": (3, 1),
          "gathers of more than MT_GT_CH chunks": (4, 0), "gathers of exactly MT_GT_CH chunks": (4, 1),
          "calls with >= 3 gathers": (5, 0), "gathers after a gather, call over >= 3 leaves (packParent)": (5, 1),
          "gathers after a gather and a run extended in place": (6, 0), "new-region gathers right after a slack gather": (6, 1),
          "compactions by a run's plan after a gather in the call": (7, 0), "heads that lose MT_M_NONL": (7, 1)}
NAMES = list(LAYOUT)


def counts(prof):
    """{counter name: total} of an array [documents, 8] of prof slots (two 32-bit counters a slot)."""
    prof = np.asarray(prof, np.uint64)
    return {nm: int(((prof[:, s] >> np.uint64(32 * hi)) & np.uint64(0xFFFFFFFF)).sum()) for nm, (s, hi) in LAYOUT.items()}


def build(flag="MT_EVGATHER"):
    lib = os.path.join(tempfile.gettempdir(), f"libmtemu_{flag.lower()}_{os.getuid()}.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-D" + flag,
                           "-o", lib, os.path.join(ROOT, "tests", "emu", "mt_emu.cpp")])
    return lib


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "config2"
    docs = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    res = sys.argv[3] if len(sys.argv) > 3 else "blk"
    c = dict(bench.CONFIGS[cfg]); c["docs"] = docs
    eng = Engine(docs, lib_path=build(), prefix="emu_", **bench.caps_for(c))
    eng.set_residency(bench.RESIDENCY[res])
    eng.upload_props(bench.ann_props()); eng.upload_names(['"c%d"' % i for i in range(64)])
    p = MtGenParams(7, docs, c["ops"], c["clients"], c["lag"], c["ins"], c["rem"], c["ins_len"], c["rem_len"],
                    c["ann_sets"], c["rewrite"])
    eng.generate(p); eng.sync(); eng.generated_to_resident(); eng.open_docs(0, docs)
    fn = eng.lib.emu_prof_get; fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    base = np.zeros((docs, 8), np.uint64); fn(eng.h, docs, base.ctypes.data)
    eng.replay_resident(); eng.sync()
    raw = np.zeros((docs, 8), np.uint64); fn(eng.h, docs, raw.ctypes.data)
    msgs = float(docs * c["ops"])
    t = counts(raw - base)
    print(f"{cfg} docs={docs} res={res} msgs={int(msgs)}")
    for nm in NAMES:
        print(f"  {nm:58s} {t[nm]:10d}  {t[nm] / msgs:8.4f} per message")
    g = max(t["gathers"], 1)
    print(f"  share of gathers with an earlier gather in the same scourLeaves call: {t[AFTER] / g:.4f}")
    print(f"  mean 64-unit chunks per gather: {t['64-unit chunks'] / g:.3f}   mean units per gather: {t['units'] / g:.1f}")
    print(f"  gathers per scourLeaves call that gathers: {g / max(t['calls with a gather'], 1):.3f}")


if __name__ == "__main__":
    main()
