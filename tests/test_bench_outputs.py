"""bench.py's plain run and `--dump-outputs`: the dumped arrays' format on the CPU (float32, rejected
reports' prep messages zeroed, the size cap and its seeded sample), the inputs-only pool being the
full pool's inputs, and on the GPU one plain run whose dumped outputs are checked against the oracle.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _fake(n, seed=1):
    rng = np.random.default_rng(seed)
    verdicts = (rng.integers(0, 10, n) == 0).astype(np.uint8) * 3
    msgs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    share = (bytes(rng.integers(0, 256, 48, dtype=np.uint8)), 1234567, bytes(range(32)))
    merged = (bytes(rng.integers(0, 256, 48, dtype=np.uint8)), 2 * 1234567, bytes(range(32, 64)))
    return verdicts, msgs, share, merged


def test_dump_outputs_format(tmp_path):
    verdicts, msgs, share, merged = _fake(1000)
    files = bench.dump_outputs(str(tmp_path), verdicts, msgs, share, merged)
    assert sorted(files) == sorted(f[:-4] for f in os.listdir(tmp_path))
    got = {k: np.load(tmp_path / f"{k}.npy") for k in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert "rows" not in got
    assert np.array_equal(got["verdicts"], verdicts)
    words = got["prep_msgs"].astype("<u2")
    assert got["prep_msgs"].shape == (1000, 8) and np.array_equal(words, got["prep_msgs"])  # exact in float32
    back = words.view(np.uint8)
    ok = verdicts == 0
    assert 0 < ok.sum() < 1000
    assert np.array_equal(back[ok], msgs[ok]) and not back[~ok].any()
    assert bytes(got["aggregate_share"].astype(np.uint8)) == share[0]
    assert got["report_count"].dtype == np.float64 and got["report_count"][0] == share[1]
    assert bytes(got["checksum"].astype(np.uint8)) == share[2]
    assert bytes(got["merged_aggregate_share"].astype(np.uint8)) == merged[0]
    assert got["merged_report_count"][0] == merged[1]
    # without a combine in the step there is no merged record to write
    files = bench.dump_outputs(str(tmp_path / "own"), verdicts, msgs, share, None)
    assert not any(k.startswith("merged_") for k in files)


def test_dump_outputs_cap_and_sample(tmp_path, monkeypatch):
    # the default step (1.25M reports) is kept whole and stays under 64 MB; the cap itself does too
    per_row, per_row_sampled = 4 + 8 * 4, 4 + 8 * 4 + 8
    assert 1_250_000 <= bench.DUMP_MAX_ROWS
    assert bench.DUMP_MAX_ROWS * per_row_sampled + 2 * (16 * 1000 + 32 + 2) * 4 + 7 * 128 < 64 * 10**6
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 100)
    verdicts, msgs, share, _ = _fake(1000)
    bench.dump_outputs(str(tmp_path / "a"), verdicts, msgs, share, None)
    bench.dump_outputs(str(tmp_path / "b"), verdicts, msgs, share, None)
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and rows.shape == (100,) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))  # fixed seed: the same rows every run
    assert np.array_equal(np.load(tmp_path / "a" / "verdicts.npy"), verdicts[rows.astype(np.int64)])
    assert np.load(tmp_path / "a" / "prep_msgs.npy").shape == (100, 8)
    assert per_row == 36


def test_inputs_only_pool_is_the_full_pool(tmp_path, monkeypatch):
    from janus_amd.vdaf import Prio3

    monkeypatch.setenv("JX_POOL_CACHE", str(tmp_path))
    vdaf, vk, K = Prio3.sum_vec(1, 7, 3), bytes(range(16)), 130
    _, *plain, want, how = bench.load_or_make_pool(vdaf, vk, K, 2, 0, expect=False)
    assert want is None and how == "generated"
    _, *again, want, how = bench.load_or_make_pool(vdaf, vk, K, 2, 0, expect=False)
    assert want is None and how == "cached" and all(np.array_equal(a, b) for a, b in zip(plain, again))
    _, *full, want, how = bench.load_or_make_pool(vdaf, vk, K, 2, 0, expect=True)
    assert how == "generated" and want["count"] == K - 2 and len(want["blocks"]) == 1
    assert all(np.array_equal(a, b) for a, b in zip(plain, full))
    # a plain run reuses a full pool file that is already there
    os.remove(bench.pool_cache_path(vdaf, vk, K)[:-4] + "_inputs.npz")
    _, *reuse, want, how = bench.load_or_make_pool(vdaf, vk, K, 2, 0, expect=False)
    assert want is None and how == "cached" and all(np.array_equal(a, b) for a, b in zip(full, reuse))


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plain_run_dumps_what_the_step_computed(tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR` on a small step: the plain line carries the
    headline fields and none of the --full blocks, and the dumped verdicts, prep messages, aggregate share
    and merged record equal the oracle's for the same seeded pool (3 accumulated steps of R reports)."""
    from janus_amd.vdaf import Prio3

    R, K, steps, warmup = 3000, 300, 2, 1
    env = dict(os.environ, JX_POOL_CACHE=str(tmp_path))
    out_dir = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--reports-per-gpu", str(R), "--pool", str(K), "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "reports/s" and line["higher_is_better"] is True
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 / R - 1) < 1e-3
    assert line["kernels"]["k1_xof_ms_per_launch"] > 0
    assert not {"verified", "verification", "roofline", "cpu_baseline", "secondary"} & set(line)
    assert sorted(line["outputs"]["files"]) == sorted(f[:-4] for f in os.listdir(out_dir))

    vdaf, vk = Prio3.sum_vec(8, 1000, 88), bytes(range(16))
    orc, nonces, ps, his, lps, want = bench.make_pool(vdaf, vk, K, threads=8)
    idx = np.arange(R) % K
    got = {k: np.load(out_dir / f"{k}.npy") for k in line["outputs"]["files"]}
    assert np.array_equal(got["verdicts"], want["verdicts"][idx])
    fin = want["verdicts"][idx] == 0
    assert 0 < (~fin).sum() < R
    msgs = got["prep_msgs"].astype("<u2").view(np.uint8)
    assert np.array_equal(msgs[fin], want["prep_msgs"][idx][:, :16][fin]) and not msgs[~fin].any()
    cyc = bench.CyclicPool(want["verdicts"] == 0, [bench.field_elems(b.tobytes(), 16) for b in want["blocks"]],
                           bench.POOL_BLOCK, lambda a, r: bench.field_elems(
                               orc.helper_prep_batch(vk, nonces[a:r], ps[a:r], his[a:r], lps[a:r])["agg"], 16), bench.P128)
    exp_agg, exp_count = cyc.range(0, R, steps + warmup)
    exp_bytes = b"".join(x.to_bytes(16, "little") for x in exp_agg)
    for prefix in ("", "merged_"):  # one rank: the merged shard record is the rank's own
        assert bytes(got[prefix + "aggregate_share"].astype(np.uint8)) == exp_bytes
        assert got[prefix + "report_count"][0] == exp_count
