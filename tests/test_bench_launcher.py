"""bench.py's multi-GPU path on CPU: `--gpus 2` starts two ranks under
torch.distributed.run, each replays its own documents (config 2: weak scaling, gloo
barrier, max-over-ranks time) or its LPT share after rank 0's ingest (config 5:
all_to_all redistribution + digest gather to rank 0), and rank 0 prints one JSON line
with n_gpus 2.  At N=1 the line carries the digest parity check against the oracle.
Runs bench's code on the host emulation (tests/bench_emu_driver.py)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "bench_emu_driver.py")


def run(*args, timeout=300, full=True):
    """One bench line from the emulation driver; the parity checks, the CPU baseline and the
    digests these tests read are behind --full."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, DRIVER, *args, *(["--full"] if full else [])], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_launcher_config2_two_ranks():
    out = run("--gpus", "2", "--config", "config2", "--docs", "3", "--ops", "400", "--steps", "2", "--warmup", "1",
              "--no-cpu-baseline")
    assert out["n_gpus"] == 2 and out["scaling"] == "weak"
    # every rank replays its own sample on the oracle; rank 0 reports the sum (N > 1 parity)
    assert out["parity"].startswith("SnapshotV1 digests == oracle on 6 docs (2 ranks"), out["parity"]
    assert out["value"] > 0 and out["steps"] == 2


def test_launcher_config5_two_ranks():
    out = run("--gpus", "2", "--config", "config5", "--docs", "5", "--steps", "1", "--warmup", "0",
              "--no-cpu-baseline")
    assert out["n_gpus"] == 2
    assert out["config"]["docs_total"] == 10
    assert out["parity"].startswith("status words clean on every rank")
    assert out["exchange"]["docs_checked"] == 10 and out["exchange"]["checksum_mismatch_docs"] == 0


def test_launcher_config5_two_ranks_oracle_parity():
    out = run("--gpus", "2", "--config", "config5", "--docs", "6", "--steps", "1", "--warmup", "0")
    assert out["n_gpus"] == 2 and out["config"]["docs_total"] == 12
    assert out["parity"].startswith("SnapshotV1 digests == oracle on 12 docs (2 ranks"), out["parity"]
    assert out["exchange"]["checksum_mismatch_docs"] == 0


def test_single_rank_digest_parity_against_oracle():
    out = run("--config", "config2", "--docs", "20", "--ops", "300", "--steps", "1", "--warmup", "0",
              "--cpu-seconds", "0.2")
    assert out["n_gpus"] == 1
    assert out["parity"].startswith("SnapshotV1 digests == oracle on"), out["parity"]
    assert out["cpu_baseline"]["kind"] == "port"
    assert out["roofline"]["bytes_pinned"].startswith("mt_doc_counters == oracle"), out["roofline"]


def test_config5_rank_shares_equal_one_rank_replay():
    """--shares 4: the four ranks' LPT shares of 20 documents replayed in turn give every
    document the SnapshotV1 digest a one-rank replay of all 20 gives (each share's rows are the
    send buffer's slice all_to_all_single would deliver)."""
    sh = run("--config", "config5", "--docs", "5", "--shares", "4", "--steps", "1", "--warmup", "0", "--no-cpu-baseline")
    one = run("--config", "config5", "--docs", "20", "--steps", "1", "--warmup", "0", "--no-cpu-baseline")
    assert len(sh["shares"]) == 4 and sum(x["docs"] for x in sh["shares"]) == 20
    assert all(x["status_clean"] for x in sh["shares"])
    assert sh["config"]["msgs_total"] == one["config"]["msgs_total"]
    assert sh["digest_xor"] == one["sharding"]["digest_xor"]
    assert sh["ms_per_step"] == max(x["ms_per_step"] for x in sh["shares"])


SMALL = ("--config", "config2", "--docs", "20", "--ops", "300", "--steps", "2", "--warmup", "1")


def test_plain_run_reports_only_the_headline():
    """Without --full the line carries the timed figure (and what the timed launches themselves
    give: roofline, status words) and none of the legs that take work of their own."""
    out = run(*SMALL, full=False)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "ops/s" and out["higher_is_better"] is True and out["dtype"] == "int32"
    assert out["ms_per_step"] > 0
    # value = messages of the timed steps / their time: 20 docs x 300 msgs per step
    assert abs(out["value"] - 20 * 300 / (out["ms_per_step"] / 1e3)) <= 1e-6 * out["value"]
    assert out["parity"] == "status words clean"
    for leg in ("cpu_baseline", "ingest", "snapshot", "parity_manifest"):
        assert leg not in out, leg


def test_plain_run_of_the_other_configs_dumps_clean_documents(tmp_path):
    """Configs 4 and 5 without --full: the headline line, and --dump-outputs still writes every
    document's status word and digest (config 5: under its global document id)."""
    import numpy as np
    cases = {"config4": (3, ("--docs", "3", "--ops", "200", "--prebuild", "300")), "config5": (12, ("--docs", "12"))}
    for cfg, (n, size) in cases.items():
        d = str(tmp_path / cfg)
        out = run("--config", cfg, *size, "--steps", "2", "--warmup", "0", "--dump-outputs", d, full=False)
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["parity"].startswith("status words clean"), out["parity"]
        assert "snapshot" not in out and "cpu_baseline" not in out and "parity_manifest" not in out
        assert sorted(np.load(os.path.join(d, "docs.npy"))) == list(range(n))
        assert not np.load(os.path.join(d, "status.npy")).any()
        dg = np.load(os.path.join(d, "digests.npy"))
        assert dg.shape == (n, 2) and dg.dtype == np.float64 and dg.any(axis=1).all()


def test_dump_outputs_repeatable_and_equal_to_the_full_run(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files, the same from run to run, and the
    digests it writes are the ones the --full line reports."""
    import numpy as np
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run(*SMALL, "--dump-outputs", a, full=False)
    full = run(*SMALL, "--dump-outputs", b, "--no-ingest", "--cpu-seconds", "0.2")
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"status.npy", "counters.npy", "digests.npy", "text_units.npy", "text_lengths.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert x.shape == y.shape and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert not np.load(os.path.join(a, "status.npy")).any()
    d = np.load(os.path.join(a, "digests.npy")).astype(np.uint64)
    assert d.shape == (20, 2)
    xor = int(np.bitwise_xor.reduce((d[:, 0] << np.uint64(32)) | d[:, 1]))
    assert f"{xor:016x}" == full["snapshot"]["digest_xor"]
    assert full["parity"].startswith("SnapshotV1 digests == oracle on"), full["parity"]
    lens = np.load(os.path.join(a, "text_lengths.npy"))
    assert lens.sum() == len(np.load(os.path.join(a, "text_units.npy"))) > 0
