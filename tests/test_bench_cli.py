"""bench.py's command line and its --dump-outputs writer, without a GPU: the options parse, --steps must be positive, and
the writer's files are float64, hold a fixed particle sample and stay within 64 MB at the largest per-GPU map (config S)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_is_lean_by_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


class FakeNav:
    """the getters dump_outputs reads, over a map of `comps` components per particle"""

    def __init__(self, P, comps):
        self.P, self.comps = P, comps
        self.rng = np.random.default_rng(5)

    def sync(self):
        pass

    @property
    def VehicleWeights(self):
        return np.full(self.P, 1.0 / self.P)

    @property
    def BestParticle(self):
        return 3

    def resample_sources(self):
        return np.arange(self.P, dtype=np.int32), True

    def poses(self):
        return np.tile([0, 0, 0, 1.0, 0, 0, 0], (self.P, 1))

    def MapModel(self, i):
        k = self.comps
        return np.full(k, float(i)), np.full((k, 3), float(i)), np.tile(np.eye(3), (k, 1, 1))


@pytest.mark.parametrize("P,comps", [(2048, 600), (4096, 1024)], ids=["config-B", "config-S"])
def test_dump_outputs_files(tmp_path, P, comps):
    bench.dump_outputs(FakeNav(P, comps), str(tmp_path))
    files = {f: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(f.endswith(".npy") and a.dtype == np.float64 for f, a in files.items())
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    sample = files["map_particles.npy"]
    assert len(sample) == bench.DUMP_MAP_PARTICLES and np.all(np.diff(sample) > 0)
    assert np.array_equal(files["map_weights.npy"], np.repeat(sample, comps))   # each particle's map, in sample order
    assert files["map_covs.npy"].shape == (bench.DUMP_MAP_PARTICLES * comps, 3, 3)
    assert files["best_particle.npy"][0] == 3 and files["resampled.npy"][0] == 1
    again = tmp_path / "again"
    bench.dump_outputs(FakeNav(P, comps), str(again))
    assert np.array_equal(np.load(again / "map_particles.npy"), sample)   # the sample is fixed
