"""bench.py's command line on the GPU, at a small size: the plain run's line,
--dump-outputs (the same files from run to run, and the state and extras the
oracle computes for the same batch) and --full's legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OPS, N_KEYS, K, D = 200_000, 2048, 8, 8
SIZE = ["--n-ops", str(N_OPS), "--n-keys", str(N_KEYS), "--k", str(K), "--n-dc", str(D)]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", *SIZE, *extra], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def load_dump(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def dumps(gpu, tmp_path_factory):
    """Two plain runs with the same arguments: (line, dump) of each."""
    out = []
    for i in range(2):
        d = str(tmp_path_factory.mktemp(f"dump{i}"))
        out.append((run_bench("--dump-outputs", d), load_dump(d)))
    return out


def test_plain_line(dumps):
    line = dumps[0][0]
    for k in HEADLINE:
        assert k in line
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "ops/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N_OPS / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing beside the headline ran
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert line["detail"]["full"] is False
    assert len(line["detail"]["tier0_kernel_ms_steps"]) == 3
    for leg in ("host_entry", "steady_state", "cpu_baseline_threads", "weak_scaling"):
        assert leg not in line["detail"]


def test_dump_is_reproducible_and_bounded(dumps):
    a, b = dumps[0][1], dumps[1][1]
    assert sorted(a) == sorted(b) and "state_obs_id" in a and "key_sizes" in a and "extras" in a
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name
    assert sum(x.nbytes for x in a.values()) <= 64_000_000


def test_dump_matches_oracle(dumps):
    """The dumped state (every key at this size) and extras are the oracle's
    for the batch bench.py generates (seed 0xCC0DE+2, its generator settings)."""
    import oracle as orc
    from antidote_ccrdt_amd.engine import gen_trmv
    got = dumps[0][1]
    b = gen_trmv(N_OPS, N_KEYS, D, n_players=256, score_max=10**6, rmv_pm=100, lag_max=64, seed=0xCC0DE + 2)
    o = orc.TrmvOracle(N_KEYS, K, D)
    x = o.apply(b)
    st = o.export()
    assert np.array_equal(got["state_keys"], np.arange(N_KEYS))
    for f in orc.TRMV_FIELDS:
        want, name = st[f], "state_" + f
        if f.endswith("_ptr"):
            want, name = np.diff(want.astype(np.int64)), "state_" + f[:-4] + "_count"
        assert np.array_equal(got[name], want.astype(got[name].dtype)), f
    sizes = got["key_sizes"]
    assert sizes.shape == (4, N_KEYS)
    assert np.array_equal(sizes[1], got["state_m_count"])
    assert np.array_equal(sizes[2], got["state_r_count"])
    assert np.array_equal(sizes[3], got["state_obs_count"])
    ops = np.nonzero(x["kind"] != 255)[0]
    ex = got["extras"]
    assert int(got["extra_count"][0]) == ops.shape[0] and ex.shape == (ops.shape[0], 6 + D)
    assert np.array_equal(ex[:, 0], ops) and np.array_equal(ex[:, 1], x["kind"][ops])
    assert np.array_equal(ex[:, 2], x["id"][ops])
    add, rmv = x["kind"][ops] == 0, x["kind"][ops] == 2
    for col, f in ((3, "score"), (4, "dc"), (5, "ts")):
        assert np.array_equal(ex[add, col], x[f][ops][add]), f
    assert np.array_equal(ex[rmv, 6:], x["vc"][ops][rmv])
    assert np.array_equal(got["replica_vc"], st["vc"].max(axis=0))


def test_full_line(gpu):
    line = run_bench("--full", "--steady-batches", "1", "--cpu-sample-keys", "256", "--cpu-steady-keys", "256")
    for k in HEADLINE:
        assert k in line
    rl, det = line["roofline"], line["detail"]
    assert rl["kernel_ms"] > 0 and rl["algorithmic_bytes_per_launch"] > 0 and 0 < rl["frac"] < 1
    assert len(rl["kernel_ms_steps"]) == 3
    assert line["cpu_baseline"]["value"] > 0 and det["cpu_baseline_threads"]["value"] > 0
    assert det["host_entry"]["ops_per_s"] > 0
    assert len(det["steady_state"]["batches"]) == 1 and det["steady_state"]["cpu_baseline"]
    assert det["final_state"]["observed"] > 0
