"""bench.py's stdout contract without a GPU: the compact line built from a full record (the 20 KB record of round 5, which the
driver could not parse as one line) carries the contract's keys, the roofline and the CPU baseline as numbers, and fits the
driver's tail with room to spare; emit() puts it LAST on stdout and the full record on stderr / in bench_detail.json."""
import io
import json
import os
import sys
from contextlib import redirect_stderr, redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def _record():
    return json.load(open(os.path.join(ROOT, "profiles", "r05_bench_default.json")))


def test_compact_line_of_a_full_record():
    full = _record()
    assert len(json.dumps(full)) > 16000
    line = bench.compact_line(full)
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.COMPACT_LIMIT - 512
    for k in CONTRACT:
        assert k in line, k
    assert line["value"] == full["value"] and line["config"]["workload"].startswith("C2")
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and "traffic" in rf
    assert all(not isinstance(v, str) or len(v) < 64 for v in rf.values())
    assert line["cpu_baseline"]["kind"] == "port" and len(line["cpu_baseline"]["sample"]) <= 120
    assert line["legs"]["C3"]["frac"] == full["configs"]["C3"]["roofline"]["frac"]
    assert line["legs"]["walk_free"]["bound"] == "latency+issue"
    assert line["legs"]["sharded_world1"]["value"] == full["sharded_world1"]["value"]


def test_compact_sharded_line():
    rec = _record()["sharded_world1"]
    line = bench.compact_sharded_line(rec)
    assert len(json.dumps(line, separators=(",", ":"))) < bench.COMPACT_LIMIT - 1024
    for k in CONTRACT:
        assert k in line, k
    assert line["config"]["frames_per_step"] == 8 and line["exchange_ranks"]["ranks"] == 1
    assert line["exchange_phases_us"]["exchanges"] == 9 and line["predicted"]["reference_walk"]["frames_per_s"] > 0


def test_emit_prints_the_line_last_and_trims_if_it_must(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    full = _record()
    line = bench.compact_line(full)
    line["legs"]["padding"] = "x" * 5000                     # a line that would not fit is cut down, loudly, never printed long
    out, err = io.StringIO(), io.StringIO()
    with redirect_stdout(out), redirect_stderr(err):
        bench.emit(full, line)
    lines = [ln for ln in out.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) < bench.COMPACT_LIMIT
    rec = json.loads(lines[0])
    assert rec["value"] == full["value"] and rec["roofline"] and rec["cpu_baseline"]
    assert "trimmed" in err.getvalue() and "bench.py detail: {" in err.getvalue()
    assert json.load(open(tmp_path / "bench_detail.json"))["value"] == full["value"]


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_has_no_legs_and_full_has_them_all(monkeypatch, capsys):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.leg_set == set() and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert _args(monkeypatch, "--full").leg_set == set(bench.ALL_LEGS)
    assert _args(monkeypatch, "--full", "--legs", "cpu,raycast").leg_set == {"cpu", "raycast"}
    assert _args(monkeypatch, "--full", "--no-cpu-baseline").leg_set == set(bench.ALL_LEGS) - {"cpu"}
    assert _args(monkeypatch, "--legs", "none").leg_set == set()
    for argv in (("--legs", "cpu"), ("--gpus", "2", "--dump-outputs", "d"), ("--sharded", "--dump-outputs", "d")):
        try:
            _args(monkeypatch, *argv)
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError(argv)
    assert "add --full" in capsys.readouterr().err


class _FakeTable:
    """The read-back surface dump_outputs uses, over a host model: n blocks in a shuffled hash table and heap."""

    def __init__(self, n, visible):
        import numpy as np
        from voxelhashing_demo_amd import ENTRY_DTYPE, VOXEL_DTYPE
        rng = np.random.default_rng(1)
        pos = rng.choice(64 ** 3, n, replace=False)
        self.pos = np.stack([pos // 4096 - 32, pos // 64 % 64 - 32, pos % 64 - 32], 1).astype(np.int32)
        self.ht = np.zeros(3 * n, ENTRY_DTYPE)
        self.ht["ptr"] = -1
        slots, heap = rng.permutation(3 * n)[:n], rng.permutation(n)
        self.ht["pos"][slots], self.ht["ptr"][slots] = self.pos, 512 * heap
        self.vol = np.zeros(512 * n, VOXEL_DTYPE)
        for p, h in zip(self.pos, heap):          # a block's voxels are a function of its position only
            self.vol["sdf"][512 * h:512 * h + 512] = p.sum() + np.arange(512) / 512.0
            self.vol["weight"][512 * h:512 * h + 512] = 1 + abs(p[0])
        self.visible = self.ht[slots[:visible]]

    def synchronize(self):
        pass

    def hash_table(self):
        return self.ht.copy()

    def compact(self):
        return self.visible.copy()

    def block_voxels(self, ptr):
        return self.vol[ptr:ptr + 512].copy()


def _load(d):
    import numpy as np
    return {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}


def test_dump_outputs_sorted_and_complete(tmp_path):
    import numpy as np
    t = _FakeTable(300, 40)
    shapes = bench.dump_outputs(str(tmp_path), t)
    out = _load(tmp_path)
    assert shapes == {k: list(v.shape) for k, v in out.items()}
    assert set(out) == {"blocks_pos", "visible_pos", "voxels_pos", "voxels_sdf", "voxels_weight"}
    assert all(v.dtype == np.float32 for v in out.values())
    want = t.pos[np.lexsort((t.pos[:, 2], t.pos[:, 1], t.pos[:, 0]))].astype(np.float32)
    assert np.array_equal(out["blocks_pos"], want) and np.array_equal(out["voxels_pos"], want)
    assert len(out["visible_pos"]) == 40
    assert np.array_equal(out["voxels_sdf"][:, 0], want.sum(1)) and np.array_equal(out["voxels_weight"][:, 7], 1 + abs(want[:, 0]))


def test_dump_outputs_samples_beyond_its_caps_with_a_fixed_seed(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_VOXEL_BLOCKS", 50)
    monkeypatch.setattr(bench, "DUMP_POS_ROWS", 120)
    t = _FakeTable(300, 200)
    bench.dump_outputs(str(tmp_path / "a"), t)
    bench.dump_outputs(str(tmp_path / "b"), _FakeTable(300, 200))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert len(a["voxels_pos"]) == 50 and len(a["blocks_pos"]) == 120 and len(a["visible_pos"]) == 120
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert set(map(tuple, a["voxels_pos"])) <= set(map(tuple, t.pos.astype(np.float32)))
    assert np.array_equal(a["voxels_sdf"][:, 0], a["voxels_pos"].sum(1))
    assert (np.diff(a["voxels_pos"][:, 0]) >= 0).all()
