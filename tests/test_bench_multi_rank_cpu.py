"""CPU, two ranks under gloo: bench.py's N > 1 control flow — the launch contract (`python -m torch.distributed.run --nproc-per-node N bench.py
--gpus N ...`, RANK / LOCAL_RANK / WORLD_SIZE from the environment), per-rank seeds and term counts (2^24 / N by default), the closed-form
check over ALL ranks' terms, calls in flight, barrier + max-over-ranks timing, the all_gather of the partial results and their fold, per-rank
table build times, and exactly one JSON line from rank 0 — with the library replaced by tests/bench_stub.py (DGPU_BENCH_STUB).  The driver
runs the real thing on 1 / 2 / 4 / 8 GPUs; this keeps the multi-rank path from rotting where only one GPU (or none) is at hand."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run(nproc, extra):
    env = dict(os.environ, DGPU_BENCH_STUB="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1", "--master-port", str(_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(nproc)] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                                   # rank 0 prints ONE line
    return json.loads(lines[0])


def test_two_ranks_strong_scaling_line():
    out = _run(2, ["--full", "--steps", "4", "--warmup", "1", "--log2n", "10", "--inflight", "3"])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["warmup"] == 1 and out["scaling"] == "strong" and out["higher_is_better"] is True
    assert out["config"]["terms_per_step"] == 2 * (1 << 10) and out["config"]["bit_exact_vs_closed_form"] is True
    assert abs(out["value"] - (2 * (1 << 10) / float(1 << 20)) / (out["ms_per_step"] * 1e-3)) / out["value"] < 2e-2      # (value is rounded to three decimals)
    assert len(out["config"]["per_key_setup_ms"]["precomputed_table_per_rank"]) == 2
    assert "cpu_baseline" not in out and "secondary" not in out and out["data"].startswith("STUB")
    # every N > 1 line of a --full run names its own denominator: the 1-GPU rate on the same 2^24 terms (None under the stub: there is no GPU to measure it on)
    assert "scaling_base" in out and out["scaling_base"] is None and "value / scaling_base" in out["scaling_base_note"]


def test_default_size_at_two_ranks_is_config_5s_share():
    """no --log2n: every N > 1 computes BASELINE config 5's 2^24 terms in total (here the stub only has to get the COUNT right)"""
    env_small = ["--steps", "1", "--warmup", "0", "--inflight", "1"]
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    src = open(spec.origin).read()
    assert "24 - lg" in src                                         # the rule the line below relies on
    # (2^23 terms per rank in pure Python integers would take minutes: the rule is asserted on the source, the flow on the small run above)
    out = _run(2, env_small + ["--log2n", "8"])
    assert out["config"]["terms_per_step"] == 512


def test_dump_outputs_holds_the_last_timed_result(tmp_path):
    """--dump-outputs DIR: the last timed step's (folded) result as DIR/msm_g1.npy — float64, the 18 result words as 36 exact 32-bit halves — and
    that result is the closed form over both ranks' seeded terms, so two builds given the same arguments compare file for file"""
    import importlib.util
    import numpy as np
    out = _run(2, ["--steps", "3", "--warmup", "0", "--log2n", "8", "--inflight", "2", "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 3
    a = np.load(tmp_path / "msm_g1.npy")
    assert a.dtype == np.float64 and a.shape == (3, 12)
    assert (a == np.floor(a)).all() and (a >= 0).all() and (a < 2.0 ** 32).all()
    w = a.reshape(18, 2).astype(np.uint64)
    words = w[:, 0] | (w[:, 1] << np.uint64(32))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    B = importlib.util.module_from_spec(spec); spec.loader.exec_module(B)
    tot = sum(B.dot_mod_r(B.seeded_scalars(0x5EED2000 + r, 1 << 8), B.seeded_scalars(0x5EED1000 + r, 1 << 8)) for r in range(2)) % B.R_MOD
    assert sum(int(words[i]) << (64 * i) for i in range(4)) == tot and int(words[12]) == 1      # (tests/bench_stub.py: a "point" is its integer, z = 1)


MOVED_BEHIND_FULL = ("stages_ms", "stages_ms_one_in_flight", "roofline", "valu_roofline", "cpu_baseline", "secondary", "scaling_base", "scaling_base_note")


def _run_one_rank(extra, dump=None):
    """one stubbed rank started directly (no launcher at N = 1): (the JSON line, stderr)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--log2n", "8", "--inflight", "2"] + extra
    r = subprocess.run(cmd, env=dict(os.environ, DGPU_BENCH_STUB="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), r.stderr


def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    """without --full: the line with the headline's keys, the dumped result, and nothing that is measured after the timed steps — the development twin
    is never entered; with --full the same line plus the stage / roofline objects and scaling_base, and the same dumped result"""
    import numpy as np
    plain, err_plain = _run_one_rank(["--dump-outputs", str(tmp_path / "plain")])
    full, err_full = _run_one_rank(["--full", "--dump-outputs", str(tmp_path / "full")])
    for k in MOVED_BEHIND_FULL:
        assert k not in plain, k
    assert "twin entered" not in err_plain and "twin entered" in err_full
    for k in ("stages_ms", "stages_ms_one_in_flight", "roofline", "scaling_base", "scaling_base_note"):
        assert k in full, k
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "data", "inflight"):
        assert plain[k] == full[k], k
    assert plain["config"]["terms_per_step"] == full["config"]["terms_per_step"] == 1 << 8 and plain["config"]["bit_exact_vs_closed_form"] is True
    for out in (plain, full):
        assert out["steps"] == 3 and out["warmup"] == 1 and out["higher_is_better"] is True and out["ms_per_step"] > 0
        assert abs(out["value"] - ((1 << 8) / float(1 << 20)) / (out["ms_per_step"] * 1e-3)) / out["value"] < 2e-2
    assert (np.load(tmp_path / "plain" / "msm_g1.npy") == np.load(tmp_path / "full" / "msm_g1.npy")).all()
