"""bench.py's plain run, --full and --dump-outputs.

CPU: the dump helpers (exact limbs, a fixed seeded sample under the size cap). GPU: a small headline run
in this process: --steps sets the timed steps, a plain run carries none of the --full figures, the
dumped fold is the ciphertext of the plaintext sum and is the same from run to run, and --full checks
the result and measures the CPU baseline."""
import json

import numpy as np
import pytest

import bench

ROWS = 5000  # more than one fold group, not a multiple of the 64-row block


def test_int_limbs_exact():
    x = (1 << 4094) + 0xFFFFFFFF_00000001
    limbs = bench.int_limbs(x, 4095)
    assert limbs.dtype == np.float64 and limbs.shape == (128,)
    assert sum(int(v) << (32 * i) for i, v in enumerate(limbs)) == x
    assert bench.int_limbs(0, 0).shape == (1,)


def test_dump_sample_is_fixed_and_capped(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP", 1000)
    small = np.arange(1000, dtype=np.uint32)
    assert np.array_equal(bench.dump_sample(small, 2), small.astype(np.float64))
    big = np.arange(5000, dtype=np.uint32) * 3
    a, b = bench.dump_sample(big, 2), bench.dump_sample(big, 2)
    assert a.dtype == np.float64 and a.shape == (1000,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a.tolist()) <= set(big.tolist())


def test_dump_cap_keeps_every_workload_under_64_mb():
    # at most 3 sampled arrays per workload (float64), beside a few thousand limbs
    assert 3 * bench.DUMP_CAP * 8 + (1 << 20) <= 64 << 20


def test_options_exist(capsys):
    with pytest.raises(SystemExit) as e:
        bench.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--full" in text and "--dump-outputs DIR" in text
    for bad in (["--gpus", "0"], ["--steps", "0"]):
        with pytest.raises(SystemExit) as e:
            bench.main(bad)
        assert e.value.code == 2


def _run(capsys, *extra):
    capsys.readouterr()
    assert bench.main(["--gpus", "1", "--rows", str(ROWS), "--warmup", "1", *extra]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_fold(capsys, tmp_path, keys):
    import ddshe
    from oracle import homo
    d = _run(capsys, "--steps", "3", "--dump-outputs", str(tmp_path / "a"))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["metric"] == "Paillier homomorphic adds/sec (2048-bit key, mod n^2)" and d["unit"] == "HomoAdd/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u32" and d["n_gpus"] == 1
    assert d["value"] == pytest.approx((ROWS - 1) / (d["ms_per_step"] / 1e3), rel=1e-9)
    # nothing beside the headline figure was measured or checked
    assert d["cpu_baseline"] is None and d["end_to_end"] is None and d["strong_split_1gpu"] is None
    assert d["verified"] is None and not {"latency", "configs", "single_process_multi_gpu"} & set(d)
    limbs = np.load(tmp_path / "a" / "sum.npy")
    assert limbs.dtype == np.float64 and limbs.shape == (128,)
    k = keys["paillier2048_committed"]
    fold = sum(int(v) << (32 * i) for i, v in enumerate(limbs))
    want = int(ddshe.synth_plaintexts(2, 0, ROWS).astype("int64").sum()) % k["n"]
    assert 0 < fold < k["nsquare"] and homo.paillier_decrypt(fold, k) == want
    # the same arguments give the same inputs, so the same output, whatever the number of steps
    _run(capsys, "--steps", "1", "--dump-outputs", str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "sum.npy"), limbs)


@pytest.mark.gpu
def test_full_run_checks_and_measures_the_baseline(capsys):
    d = _run(capsys, "--steps", "2", "--full", "--no-extras", "--no-e2e", "--cpu-seconds", "0.05")
    assert d["steps"] == 2 and d["verified"] is True
    assert d["cpu_baseline"]["gpu_matches_sample"] is True and d["cpu_baseline"]["value"] > 0
