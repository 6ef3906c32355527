"""tests/raycast_ref.py (the DDA raycast's rule in numpy, written from DESIGN.md 4.6) against the oracle (vho_raycast_dda, with
and without jumps) on every crafted view of tests/raycast_cases.py, and the census: the conditions, computed by the reference
alone, without which the GPU tests of tests/test_gpu_raycast_crafted.py could pass vacuously.  Run with -s for the census.

Outcome of reference against oracle: no disagreement.  Depth and normals are bit-equal in every case, both with and without
jumps, also in the three cases compared under the NaN rule (their NaNs come out with the same sign and payload on this host, which
the rule does not ask for)."""
import numpy as np
import pytest

import mesh_models as mm
import raycast_cases as rc
import raycast_ref


@pytest.fixture(scope="module")
def refs(oracle):
    return {case.name: rc.reference(case, oracle) for case in rc.CASES}


def of_kind(kind):
    return [c for c in rc.CASES if kind in c.kinds]


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_reference_equals_oracle(oracle, refs, case):
    depth, normals, record = refs[case.name]
    print("\n" + rc.census_line(case, depth, record))
    ot = oracle.OracleTable(oracle.default_params(voxelSize=rc.VS, **rc.TABLES["a"]), case.W, case.H, 1)
    ot.set_raycast_intrinsics(case.focal, case.focal, case.cx, case.cy)
    assert ot.import_view(mm.view_records(case.model)) == 0
    for jumps in (False, True):
        od, on = ot.raycast(case.pose, *case.t, jumps=jumps, normals=True)
        assert rc.same_image(od, depth, case.nan), jumps
        assert rc.same_image(on, normals, case.nan), jumps
    ot.close()


def test_reduced_models_equal_the_oracle_after_deletion(oracle):
    """Variant (d): the reference of the reduced model is what the oracle renders after vho_delete_blocks."""
    for case in (c for c in rc.CASES if "d" in c.tables):
        gone = rc.deleted_keys(case.model)
        assert len(case.model) / 5 < len(gone) < len(case.model) / 2
        depth, normals, record = rc.reference(case, oracle, rc.reduced(case.model))
        ot = oracle.OracleTable(oracle.default_params(voxelSize=rc.VS, numVoxelBlocks=rc.POOL, **rc.TABLES["d"]), case.W, case.H, 1)
        ot.set_raycast_intrinsics(case.focal, case.focal, case.cx, case.cy)
        assert ot.import_view(mm.view_records(rc.reduced(case.model))) == 0
        od, on = ot.raycast(case.pose, *case.t, normals=True)
        assert rc.same_image(od, depth, False) and rc.same_image(on, normals, False)
        print(f"\n{case.name}: {len(gone)} of {len(case.model)} blocks deleted, hits={record['found'].mean():.2f}")
        assert record["found"].mean() >= 0.25
        ot.close()


def test_census_ties_and_inactive_axes(refs):
    views = of_kind("tie")
    total = {k: sum(int((refs[c.name][2][k] > 0).sum()) for c in views) for k in ("tie_xy", "tie_xz", "tie_yz", "tie_xyz")}
    one = sum(int((refs[c.name][2]["inactive"] == 1).sum()) for c in views)
    two = sum(int((refs[c.name][2]["inactive"] == 2).sum()) for c in views)
    print(f"\n{len(views)} tie views: rays with a tie {total}, with one inactive axis {one}, with two {two}")
    assert min(total.values()) >= 8 and one >= 8 and two >= 8
    # ... and ties that matter to a block: with a boundary camera the rays of even pixel offsets cross all three axes at the
    # wall's entry face (t = 1/4)
    for c in of_kind("wall"):
        r = refs[c.name][2]
        assert r["found"].mean() >= 0.9
        if c.name.endswith("b"):
            assert (r["tie_xyz"] > 0).mean() >= 0.2


def test_census_walls_in_closed_form(refs):
    """A wall faces its camera: the depth of a hit is the distance of the plane, whatever the pixel, to within a voxel in
    float64 (in fact to rounding: the pair is always two voxels one step apart on the view axis)."""
    for c in of_kind("wall"):
        depth, _, r = refs[c.name]
        axis, sign = rc.AXES[c.facts["view"]]
        want = sign * (c.facts["p0"] * rc.VS - float(c.pose[axis, 3]))
        err = np.abs(depth.astype(np.float64)[r["found"]] - want).max()
        print(f"\n{c.name}: plane at depth {want:.6f} m, largest error {err / rc.VS:.2e} voxels")
        assert 0.25 < want < 0.4 and err <= rc.VS


def test_census_noise_views(refs):
    for c in of_kind("noise"):
        depth, _, r = refs[c.name]
        f = r["found"]
        assert f.mean() >= 0.25, c
        assert (r["candidates"][f] >= 2).mean() >= 0.10, c
        assert r["straddles"].sum() / f.sum() >= 0.05, c


def test_census_ranges(refs):
    (starts,), (ends,), (event,) = of_kind("starts"), of_kind("ends"), of_kind("event")
    assert refs[starts.name][2]["starts_in_allocated"].mean() >= 0.5
    # (counted among the rays that are still walking at t_max: a ray that has its hit does not get there)
    r = refs[ends.name][2]
    assert (r["ends_in_allocated"] & ~r["found"]).sum() >= 8
    r = refs[event.name][2]
    assert (r["tmax_equals_event"] & ~r["found"]).sum() >= 8
    assert (refs["range t_min 0"][2]["start"] == np.floor(rc.front_camera(starts.model, "+z", 8))).all()      # every ray starts in the camera's voxel


def test_census_values(refs):
    for c in of_kind("holes"):
        r = refs[c.name][2]
        assert r["normal_starved"].sum() >= 1 and r["normal_one_sided"].sum() >= 1, c
        assert (refs[c.name][1][r["normal_starved"]] == 0).all()
    depth = refs["non_finite"][0]
    assert np.isnan(depth).sum() >= 1 and (np.isfinite(depth) & (depth != 0)).sum() >= 1
    assert (refs["weights"][2]["broken_by_weight"] > 0).sum() >= 1
    d, n, r = refs["zero_gradient"]
    assert r["found"].mean() >= 0.25 and not n.any()                           # hits, and not one normal
    d, n, r = refs["zeros"]                                                     # +0 and -0 as the pair's second sample
    _, second, _ = raycast_ref.Field(rc.BY_NAME["zeros"].model).voxels(r["hit"][r["found"]])
    bits = set(second.view(np.uint32).tolist())
    assert 0 in bits and 0x80000000 in bits


def test_census_forms(refs):
    """Which traversal the forced cooperative launch runs.  At fx = 32 a patch's beam is wider than two blocks beyond about half a
    metre, so the crafted views end there: in every case but the ones named here some patches have no wide box (over all of
    them: most), few cells are listed, no block lies far from the first -- the cooperative walk itself renders those.  The named ones are there for the fall-backs:
    wide boxes (the `deep` views), set overflow alone (`long beam`, crowded table), a far block alone (`two clusters`)."""
    plain = []
    for c in rc.CASES:
        for table in c.tables:
            cells, wide = rc.beam_cells(c, rc.TABLES[table]["numBuckets"], rc.reduced(c.model) if table == "d" else None)
            print(f"\n{c.name} ({table}): cells with a set bit per patch {min(cells)}..{max(cells)}, patches with a wide box {sum(wide)} of {len(wide)}")
            if "deep" in c.kinds or c.name == "far":          # (far: the boxes' margin grows with the coordinates, 10 voxels at 2^20)
                assert all(wide)
            elif "overflow" in c.kinds:
                assert not any(wide) and min(cells) > 256
            elif "far_block" in c.kinds:
                assert not any(wide) and max(cells) <= 128
            else:            # (wide at the image's edges and where the camera looks along a block face: a slab also moves sideways)
                assert not all(wide) and max(cells) <= 128
                plain += [w for w in wide]
    print(f"\nviews for the cooperative walk: {sum(plain)} of {len(plain)} patches have a wide box")
    assert sum(plain) < len(plain) / 2
    for c in (c for c in rc.CASES if "b" in c.tables):
        bucket = mm.hash_block(list(c.model), rc.TABLES["b"]["numBuckets"])
        assert np.bincount(bucket).max() >= 2 and len(set(bucket.tolist())) >= 6      # keys behind a bucket's first slot, many bits set
    r = refs["long beam"][2]
    span = (r["hit"][..., 2] >> 3) - (r["start"][..., 2] >> 3)
    assert r["found"].mean() >= 0.25 and 256 < span[r["found"]].min() and span[r["found"]].max() < 500
    c = rc.BY_NAME["two clusters"]
    r = refs[c.name][2]
    span = (r["hit"][..., 2] >> 3) - (r["start"][..., 2] >> 3)
    print(f"\n{c.name}: hits={r['found'].mean():.2f}, the hit block is {span[r['found']].min()}..{span[r['found']].max()} blocks behind the ray's first")
    assert r["found"].mean() >= 0.25 and span[r["found"]].min() > 511
