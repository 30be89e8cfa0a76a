"""bench.py's command line: a plain run does the headline's work only (set-up, warm-up, exactly
--steps timed steps, one result line), --full adds the checks and side measurements, and
--dump-outputs writes the pictures of the last timed step, the same from run to run."""
import contextlib
import io
import json

import numpy as np
import pytest

from tests.test_bench_dist import _CpuHw, _OraclePipeline

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_KEYS = {"verified", "per_rank", "stage_ms", "stage_gbs", "roofline", "stage_roofline", "two_frames_in_flight",
             "film_grain_8k10", "intra_1080p8", "end_to_end_4k10", "mc_coherent_4k10", "output_4k10", "real_streams",
             "cpu_baseline"}


class _CountingPipeline(_OraclePipeline):
    made = []

    def __init__(self, fr):
        super().__init__(fr)
        self.steps = 0
        _CountingPipeline.made.append(self)

    def step(self, stream, ev=None, mark=None):
        self.steps += 1
        super().step(stream, ev, mark)

    def outputs(self, prefix=""):
        return {prefix + "y": np.full((4, 6), self.steps, np.uint16)}


class _CountingHw(_CpuHw):
    def pipeline(self, ctx, fr, ring):
        return _CountingPipeline(fr)


def _run(argv, hw):
    import bench
    _CountingPipeline.made = []
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = bench.main(argv, hw=hw)
    assert rc == 0
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_steps_and_nothing_else(monkeypatch, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = _run(["--gpus", "1", "--steps", "3", "--warmup", "2", "--frame", "128x64",
                "--dump-outputs", str(tmp_path)], _CountingHw())
    assert HEADLINE_KEYS <= set(out) and not FULL_KEYS & set(out)
    assert out["steps"] == 3 and out["warmup"] == 2 and out["full"] is False
    assert out["unit"] == "Mpixels/s" and out["higher_is_better"] is True and out["dtype"] == "u16"
    # value and ms_per_step describe the same timed region: one 128x64 frame per step
    assert out["value"] == pytest.approx(128 * 64 / (out["ms_per_step"] / 1e3) / 1e6, rel=1e-2)
    # one pipeline, warm-up + timed steps and not one more
    assert [p.steps for p in _CountingPipeline.made] == [2 + 3]
    got = np.load(tmp_path / "y.npy")
    assert got.dtype == np.float32 and np.array_equal(got, np.full((4, 6), 5, np.float32))


def test_full_run_adds_the_checks(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--frame", "128x64", "--full", "--no-fg",
                "--no-intra", "--no-extra", "--no-cpu-baseline"], _CountingHw())
    assert HEADLINE_KEYS <= set(out) and out["full"] is True and out["steps"] == 2
    assert out["verified"] is True and out["per_rank"][0]["verified"] is True
    assert set(out["stage_ms"]) == {"lr"} and out["two_frames_in_flight"]["outputs_match_sequential"] is True
    assert len(_CountingPipeline.made) == 2          # the second frame in flight


def test_dump_outputs_whole_and_sampled(tmp_path):
    import bench
    rng = np.random.default_rng(7)
    arrays = {"y": rng.integers(0, 1024, (64, 96), dtype=np.uint16), "u": rng.integers(0, 1024, (32, 48), dtype=np.uint16)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "whole" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, a)
    # over the budget: the same fraction of every array, the same positions in every run
    budget = 4 * (64 * 96 + 32 * 48) // 4
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    total = 0
    for k, a in arrays.items():
        x, y = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, y) and x.size == a.size // 4
        assert np.isin(x, a).all()
        total += x.nbytes
    assert total <= budget
    assert bench.DUMP_BUDGET <= 64 * 10 ** 6


@pytest.mark.gpu
def test_dump_outputs_is_the_timed_picture(gpu, tmp_path, monkeypatch):
    """Two plain runs with the same arguments write the same arrays, and they are the oracle's
    reference picture for the bench's own descriptors."""
    import bench
    from rav1d_amd.synth import make_frame
    from tests.pipeline import oracle_pipeline
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    w, h = 640, 360
    for d in ("a", "b"):
        out = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--frame", f"{w}x{h}",
                    "--dump-outputs", str(tmp_path / d)], bench.CudaHw())
        assert out["steps"] == 2 and not FULL_KEYS & set(out)
    fr = make_frame(w, h, bench.BPC, bench.LAYOUT, seed=0x4C100001, with_fg=False, with_mc=True)
    ref = oracle_pipeline(fr)["lr"]
    for p, name in enumerate("yuv"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == ((h, w) if p == 0 else (h // 2, w // 2))
        assert np.array_equal(a, b)
        assert np.array_equal(a, ref[p][:a.shape[0], :a.shape[1]])
