"""bench.py --dump-outputs: the arrays of the timed path's last step as float64 .npy files, a seeded sample of the rows above the size limit;
--steps as the number of timed steps; and what a plain run and a --full run put on the line."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _result(S, n_planes, n_cands, with_ocr=False):
    rng = np.random.default_rng(7)
    info = np.zeros(n_planes, S.PLANE_DTYPE)
    info["n_pool"] = n_cands // max(n_planes, 1)
    cands = np.zeros(n_cands, S.CAND_DTYPE)
    cands["key"] = rng.integers(0, 2**32, n_cands, dtype=np.uint64).astype(np.uint32)
    cands["score_strong"] = rng.standard_normal(n_cands)
    r = S.Result(info, cands, np.zeros(7), {})
    if with_ocr:
        r.ocr_label = np.arange(n_cands, dtype=np.int32)
        r.ocr_prob = rng.random(n_cands)
    return r


def test_dump_writes_every_field_as_float64(S, tmp_path):
    B = _bench()
    res = _result(S, 3, 30, with_ocr=True)
    names = B.dump_outputs(res, str(tmp_path))
    assert sorted(names) == sorted(os.path.splitext(f)[0] for f in os.listdir(tmp_path))
    fields_c = [f for f in S.CAND_DTYPE.names if f not in B.DUMP_PAD_FIELDS]
    fields_p = [f for f in S.PLANE_DTYPE.names if f not in B.DUMP_PAD_FIELDS]
    assert set(names) == {f"cands_{f}" for f in fields_c} | {f"planes_{f}" for f in fields_p} | {"ocr_label", "ocr_prob"}
    for n in names:
        assert np.load(tmp_path / f"{n}.npy").dtype == np.float64, n
    assert np.array_equal(np.load(tmp_path / "cands_key.npy"), res.cands["key"].astype(np.float64))      # u32 keys: exact in float64
    assert np.array_equal(np.load(tmp_path / "cands_score_strong.npy"), res.cands["score_strong"])
    assert np.array_equal(np.load(tmp_path / "ocr_prob.npy"), res.ocr_prob)


def test_dump_samples_the_same_rows_above_the_limit(S, tmp_path):
    B = _bench()
    res = _result(S, 4, 5000, with_ocr=True)
    limit = 64 << 10
    names = B.dump_outputs(res, str(tmp_path / "a"), limit=limit)
    B.dump_outputs(res, str(tmp_path / "b"), limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") - 128 for n in names)      # (128 = the .npy header of a 1-D array)
    assert 0 < total <= limit
    for n in names:                                                       # seeded: the same rows on every run
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")), n
    rows = np.load(tmp_path / "a" / "cands_row.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "a" / "ocr_label_row.npy"))     # per-candidate arrays keep the same rows
    assert 0 < len(rows) < 5000 and (np.diff(rows) > 0).all()
    assert np.array_equal(np.load(tmp_path / "a" / "cands_key.npy"), res.cands["key"][rows].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "ocr_label.npy"), rows.astype(np.float64))


@pytest.mark.gpu
def test_bench_dump_is_what_the_timed_path_returns(S, cascade_paths, tmp_path):
    """Three timed steps of two frames: the line says three steps of one batch, and the dump equals one call of the library on the same frames."""
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames-per-gpu", "2",
           "--pipelines", "1", "--no-cpu-baseline", "--no-latency", "--no-host-frames", "--no-ties-leg", "--no-ocr-legs", "--no-4k-leg",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["repeats"] == 1 and d["config"]["batches_per_step"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3 / 1e3)) / d["value"] < 0.02

    frames = np.stack([S.synth.stext_bgr(S.synth.frame_seed(i), W, H) for i in range(2)])
    f = S.ERFilter(params=S.Params(max_width=W, max_height=H, max_frames=2, n_pyr_levels=8, channel_mask=0x07))
    f.load_cascade(0, cascade_paths[0])
    f.load_cascade(1, cascade_paths[1])
    ref = f.text_detect(frames)
    f.close()
    assert len(ref.cands) > 0
    for name, a in (("cands", ref.cands), ("planes", ref.info)):
        for fld in a.dtype.names:
            p = out / f"{name}_{fld}.npy"
            if fld in ("r0", "r1", "r2", "reserved"):
                assert not p.exists()
                continue
            assert np.array_equal(np.load(p), a[fld].astype(np.float64)), (name, fld)


HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                 "repeats", "value_min", "value_max", "config", "nms_ties"}


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_bench_line_plain_and_full(full):
    """A plain run measures nothing beyond its timed steps -- no leg runs although none is switched off; --full adds the per-kernel-group
    times, the rooflines and the legs that are not switched off (here the S-ties leg and the latency leg)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames-per-gpu", "2", "--pipelines", "1"]
    if full:
        cmd += ["--full", "--no-cpu-baseline", "--no-host-frames", "--no-ocr-legs", "--no-4k-leg"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    extra = {"nms_ties_leg", "latency_1frame", "roofline", "tree_passes_roofline", "gpu_ms_per_step_by_kernel_group",
             "gpu_ms_per_step_by_kernel_group_serial"} if full else set()
    assert set(d) == HEADLINE_KEYS | extra
    assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    if full:
        assert d["roofline"]["avg_launch_ms"] > 0 and d["gpu_ms_per_step_by_kernel_group_serial"]
