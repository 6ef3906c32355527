"""One GPU context carried through every model-changing call of the library in a random order -- frames in every form,
de-integrations, the colour calls and the compositions, deletions and collections, vh_stream_out / vh_stream_in, vh_merge and
vh_merge_color, saved models -- with the readers in between, against the shadow model of tests/lifecycle_ref.py, which is advanced
from its own state only and never from a GPU download (a model that goes wrong but stays self-consistent does not pass).

After every model-changing step that does not deliberately leave a pipelined frame pending: every block of the model bit for bit
(key set, sdf, weight, colour word), the table's structure (lifecycle_ref.table_invariants), the call's return values and the
counters its section of the header specifies; in the crowded variant B, while no call has inserted blocks, the table slot for
slot as well.  After every reader step: its result against its rule on the SHADOW's model, and a state that equals the one
before it.  The plans and the conditions that keep them from being vacuous: tests/lifecycle_cases.py,
tests/test_lifecycle_ref_cpu.py."""
import numpy as np
import pytest

import color_ref as CR
import deintegrate_cases as DC
import esdf_ref
import lifecycle_cases as LC
import lifecycle_ref as LR
import merge_color_cases as CC
import merge_color_ref as M
import mesh_indexed_ref
import mesh_ref
import rays_ref
import sample_ref
import stream_cases as SC
import stream_ref as S

pytestmark = pytest.mark.gpu

U = np.uint32
W, H = DC.W, DC.H


def source_table(vh, seq):
    """The fixed src of the merges on the GPU: the shadow's src model handed over block by block."""
    vs = float(seq.shadow.vs)
    src = CC.table(vh, dict(DC.KW, numVoxelBlocks=2048, voxelSize=vs), seq.sem)
    st = src.stream_in(S.chunk_of(seq.src, sorted(seq.src)))
    assert st["placed"] == len(seq.src) and src.has_color()
    S.same_models(CC.model(CC.snapshot(src)), seq.src)
    return src


def keys4(torch, keys):
    k = np.zeros((len(keys), 4), np.int32)
    k[:, :3] = np.asarray(keys, np.int32).reshape(-1, 3)
    return CC.dev(torch, k)


def sorted_rows(a):
    rows = np.ascontiguousarray(a).reshape(len(a), int(np.prod(a.shape[1:]))).view(U)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def run_call(torch, gt, src, seq, step, tmp_path):
    """The step's call on the GPU context; returns what the call itself gave back."""
    op, fr, k = step["op"], seq.frames, DC.k_inv()
    dev = lambda a: CC.dev(torch, a)
    f, p, q = step.get("f"), step.get("p"), step.get("q")
    rgba = dev(CC.image(step["img"])) if "img" in step else None
    band = seq.band
    if op == "integrate_depth":
        gt.integrate_depth(fr[f][0], dev(fr[f][1]), k)
    elif op == "integrate":
        gt.integrate(fr[f][0], dev(fr[f][2]))
    elif op == "steps":
        v = dev(fr[f][2])
        gt.set_pose(fr[f][0])
        gt.reset_mutexes()
        gt.alloc_blocks(v)
        gt.flatten()
        gt.integrate_depth_map(v)
    elif op == "integrate_batch":
        gt.integrate_batch([fr[i][0] for i in step["fs"]], [dev(fr[i][2]) for i in step["fs"]])
    elif op == "deintegrate":
        gt.deintegrate(fr[p][0], dev(fr[f][2]))
    elif op == "deintegrate_depth":
        gt.deintegrate_depth(fr[p][0], dev(fr[f][1]), k)
    elif op == "integrate_color":
        gt.integrate_color(fr[f][0], dev(fr[f][1]), k, rgba, band, step["wmax"])
    elif op == "integrate_color_map":
        gt.integrate_color_map(fr[f][0], dev(fr[f][2]), rgba, band, step["wmax"])
    elif op == "deintegrate_color":
        gt.deintegrate_color(fr[p][0], dev(fr[f][1]), k, rgba, band)
    elif op == "integrate_depth_color":
        gt.integrate_depth_color(fr[f][0], dev(fr[f][1]), k, rgba, band, step["wmax"])
    elif op == "deintegrate_depth_color":
        gt.deintegrate_depth_color(fr[p][0], dev(fr[f][1]), k, rgba, band)
    elif op == "reintegrate_depth":
        gt.reintegrate_depth(fr[p][0], fr[q][0], dev(fr[f][1]), k)
    elif op == "reintegrate_depth_color":
        gt.reintegrate_depth_color(fr[p][0], fr[q][0], dev(fr[f][1]), k, rgba, band, step["wmax"])
    elif op == "delete_blocks":
        gt.delete_blocks(keys4(torch, step["keys"]))
    elif op == "garbage_collect":
        gt.garbage_collect(step["threshold"])
    elif op == "stream_out":
        return gt.stream_out(step["region"], capacity=step["capacity"])
    elif op == "stream_in":
        return gt.stream_in(step["chunk"])
    elif op in ("merge", "merge_color"):
        return gt.merge(src, step["T"], step["mode"], colors=(op == "merge_color"), color_weight_max=step["wmax"])
    elif op == "reload":
        coloured = gt.has_color()
        gt.save_snapshot(str(tmp_path / "model.snap"))
        if coloured:
            gt.save_color(str(tmp_path / "model.color"))
        gt.load_snapshot(str(tmp_path / "model.snap"))
        if step["with_color"]:
            gt.load_color(str(tmp_path / "model.color"))
    elif op == "clear_color":
        gt.clear_color()
    elif op == "set_alloc_band":
        gt.set_alloc_band(step["value"])
    else:
        gt.set_option(op, step["value"])
    return None


def check_change(gt, seq, step, got, slots):
    """The state after a model-changing step, and what the call returned, against the shadow."""
    sh, op, ex = seq.shadow, step["op"], step["expect"]
    snap = CC.snapshot(gt)
    S.same_models(CC.model(snap), sh.model())                            # every block: key set, sdf, weight, colour
    LR.table_invariants(snap, gt.params, sh.overflow)
    c = snap["counters"]
    assert c["heap_counter"] == sh.ot.heap_counter() and snap["has_color"] == ex["has_color"]
    if op not in ("reload", "clear_color"):                              # (the header leaves the list after these two open)
        assert c["occupied"] == ex["occupied"], (c["occupied"], ex["occupied"])
        assert sorted(LR.keys_of(snap["compact"])) == sorted(sh.compact)
    if slots:                                                            # no call has chosen a slot on its own yet: slot for slot
        a, b = sh.table(), snap["table"]
        assert np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["offset"], b["offset"])
        assert np.array_equal(a["ptr"] != -1, b["ptr"] != -1)
    if op in ("delete_blocks", "garbage_collect", "stream_out"):
        assert c["last_freed"] == ex["freed"]
    if op == "stream_out":
        want = ex["chunk"]
        assert got["selected"] == want["selected"] and len(got["keys"]) == len(want["keys"])
        assert (got["colors"] is None) == (want["colors"] is None)
        if slots:
            assert np.array_equal(got["keys"], want["keys"])             # the order of the table's entries
        S.same_models(SC.chunk_model(got), SC.chunk_model(want))
    if op == "stream_in":
        keys = LR.keys_of({"pos": step["chunk"]["keys"]})
        for key in set(keys):                                            # (which of two records of one key is placed is a race)
            at = [i for i, x in enumerate(keys) if x == key]
            assert sorted(got["status"][at].tolist()) == sorted(ex["status"][at].tolist()), key
        assert (got["placed"], got["present"], got["unplaced"], got["foreign"]) == (ex["placed"], ex["present"], 0, 0)
    if op in ("merge", "merge_color"):
        assert (got["candidates"], got["allocated"], got["blocks"], got["unplaced"]) == \
            (ex["stats"]["candidates"], ex["stats"]["allocated"], ex["stats"]["blocks"], 0), (got, ex["stats"])


def check_reader(torch, gt, seq, step, slots):
    """The reader's result against its rule on the shadow's model."""
    sh, op = seq.shadow, step["op"]
    dev = lambda a: CC.dev(torch, a)
    model = sh.model()
    geo = M.geometry(model)
    vs = float(sh.vs)
    if op == "raycast":
        pose = seq.frames[step["f"]][0]
        depth = torch.zeros((H, W), device="cuda")
        gt.raycast(pose, depth)
        assert np.array_equal(depth.cpu().numpy().view(U), sh.ot.raycast(pose).view(U))
    elif op == "sample_sdf":
        sdf, w = gt.sample_sdf(dev(step["points"]), step["mode"], weight=True)
        ws, ww, _ = sample_ref.sample(geo, step["points"], sh.vs, step["mode"])
        assert sample_ref.same_bits(sdf.cpu().numpy(), ws) and sample_ref.same_bits(w.cpu().numpy(), ww)
    elif op == "sample_color":
        got = gt.sample_color(dev(step["points"]), step["mode"]).cpu().numpy().view(U)
        assert np.array_equal(got, CR.sample(model, step["points"], sh.vs, step["mode"]))
    elif op == "sample_lattice":
        sdf, w = gt.sample_lattice(step["lo"], step["dims"], weight=True)
        ws, ww = sample_ref.lattice(geo, step["lo"], step["dims"])
        assert sample_ref.same_bits(sdf.cpu().numpy(), ws) and sample_ref.same_bits(w.cpu().numpy(), ww)
    elif op == "cast_rays":
        t = gt.cast_rays(dev(step["rays"]))
        assert rays_ref.same_bits(t.cpu().numpy(), rays_ref.cast(geo, vs, step["rays"])[0])
    elif op in ("mesh_count", "extract_mesh", "extract_mesh_indexed"):
        want = mesh_ref.extract(sh.table(), sh.ot.sdf_blocks(), vs, step["region"])[0]
        if op == "mesh_count":
            assert gt.mesh_count(step["region"]) == len(want)
        elif op == "extract_mesh":
            tris = gt.extract_mesh(step["region"])
            assert tris.shape == want.shape
            if slots:
                assert np.array_equal(tris.view(U), want.view(U))        # in the order of the table's entries
            assert np.array_equal(sorted_rows(tris), sorted_rows(want))
        else:
            verts, faces = gt.extract_mesh_indexed(step["region"])
            assert len(faces) == len(want) and np.array_equal(sorted_rows(verts[faces]), sorted_rows(want))
            assert len(verts) == len(mesh_indexed_ref.extract_indexed(sh.table(), sh.ot.sdf_blocks(), vs, step["region"])[0])
    elif op == "esdf_lattice":
        d = gt.esdf_lattice(step["lo"], step["dims"], step["radius"], distance=False, dist2=True)
        assert esdf_ref.same_bits(d.cpu().numpy(), esdf_ref.esdf(geo, step["lo"], step["dims"], step["radius"]))
    elif op == "stream_count":
        assert gt.stream_count(step["region"]) == sh.stream_count(step["region"])


@pytest.mark.parametrize("seed", LC.SEEDS)
@pytest.mark.parametrize("variant,sem", [(v, s) for v in ("A", "B") for s in (0, 1)])
def test_call_sequences_against_the_shadow(oracle, vh, torch_cuda, tmp_path, variant, sem, seed):
    torch = torch_cuda
    seq = LC.Sequence(oracle, variant, sem, seed)
    kw, overflow = LR.VARIANTS[variant]
    gt = CC.table(vh, kw, sem)
    if overflow:
        gt.set_option("overflow_list", 1)
    src = source_table(vh, seq)
    pending = False                                                      # a pipelined frame may be in flight
    compared = 0
    for step in seq.steps():
        op = step["op"]
        slots = variant == "B" and not seq.shadow.inserted
        try:
            if op in LC.READERS:
                before = None if pending else CC.snapshot(gt)            # (a synchronize() would launch the pending frame itself)
                check_reader(torch, gt, seq, step, slots)
                after = CC.snapshot(gt)
                if before is not None:
                    CC.unchanged(before, after)
                    assert np.array_equal(before["compact"].view(np.uint8), after["compact"].view(np.uint8))
                S.same_models(CC.model(after), seq.shadow.model())
                pending = False
            else:
                got = run_call(torch, gt, src, seq, step, tmp_path)
                pending = bool(step.get("pending"))
                if op not in LC.OPTIONS and not pending:
                    check_change(gt, seq, step, got, slots)
                    compared += 1
        except AssertionError as e:
            raise AssertionError(f"{variant} sem {sem} seed {seed}, step {step['index']} after {seq.log}: {e}") from e
    assert compared >= 15 and len(seq.shadow.live()) > 0
    S.same_models(CC.model(CC.snapshot(gt)), seq.shadow.model())
    gt.close()
    src.close()
    seq.close()
