"""The crafted cases of tests/tsdf_cases.py without a GPU: the oracle's step-level frame against the rule of
tests/deintegrate_ref.py (apply_frame, sign = +1) on every case and frame, every voxel bit, and the conditions on the inputs --
which special value is read, which stored weight is updated, which branch is taken -- counted on the reference alone, so that
tests/test_gpu_tsdf_crafted.py cannot pass by not reaching an edge."""
import numpy as np
import pytest

import deintegrate_ref as R
import tsdf_cases as TC

F = np.float32
U = np.uint32


def bits(v):
    return np.ascontiguousarray(v).view(U)


def nonfinite(c):
    return c.family == "d" or c.name.startswith("r-d")


def assert_same_voxels(want, got, c, what=""):
    """No tolerance: every bit of sdf and weight.  Where the case holds non-finite values the NaNs must stand at the same
    voxels and every other voxel is bit-equal (the payload and sign of a NaN may differ between the host and the device)."""
    assert want.shape == got.shape
    for f in ("sdf", "weight"):
        a, b = np.ascontiguousarray(want[f]), np.ascontiguousarray(got[f])
        nan = np.isnan(a)
        if not nonfinite(c):
            assert not nan.any(), (c.name, what, f, "the reference holds a NaN")
        assert np.array_equal(nan, np.isnan(b)), (c.name, what, f, "NaN positions")
        bad = np.nonzero(a.view(U)[~nan] != b.view(U)[~nan])[0]
        assert len(bad) == 0, (c.name, what, f, len(bad), a[~nan][bad[:4]], b[~nan][bad[:4]])


def load_oracle(oracle, c):
    ot = oracle.OracleTable(c.params(oracle), c.W, c.H, c.sem)
    ot.set_projection(c.proj)
    ot.set_integrate_flags(c.flags)
    keys = list(c.blocks)
    assert ot.insert_blocks(keys) == len(keys)
    tab, vol = ot.hash_table(), ot.sdf_blocks()
    where = {tuple(e["pos"].tolist()): int(e["ptr"]) for e in tab[tab["ptr"] != -1]}
    for k, (s, w) in c.blocks.items():
        vol["sdf"][where[k]:where[k] + 512], vol["weight"][where[k]:where[k] + 512] = s, w
    return ot


def key_set(entries):
    return set(map(tuple, entries["pos"].tolist()))


_runs = {}


def oracle_run(oracle, c):
    """The oracle's step-level frames of the case, once: per frame the compact list, the volume before and after, the rule's
    volume, the trace of the listed blocks and the allocated keys after the frame.  Kept and never changed."""
    if c.name in _runs:
        return _runs[c.name]
    ot = load_oracle(oracle, c)
    out = []
    for frame in c.frames:
        inv = oracle.invert4x4(frame.pose)
        ot.set_pose(frame.pose)
        ot.reset_mutexes()
        ot.alloc_blocks(frame.verts)
        ot.flatten()
        entries, pre = ot.compact().copy(), ot.sdf_blocks().copy()
        vis = R.visible_entries(ot.hash_table(), ot.params, c.sem, c.proj, frame.pose, inv, c.W, c.H)
        listed_ok = np.array_equal(ot.hash_table()[vis], entries)
        ot.integrate_depth_map(frame.depth_verts())
        want, stats = R.apply_frame(pre, entries, ot.params, c.sem, c.proj, inv, frame.pose, frame.depth_source(), c.flags, +1)
        t = TC.trace(entries, ot.params, c.sem, c.proj, inv, frame.depth_source(), c.flags)
        at = entries["ptr"].astype(np.int64)[:, None] + np.arange(512)[None, :]
        assert len(ot.allocated()) <= c.table["numVoxelBlocks"] - 8, (c.name, len(ot.allocated()))
        out.append(dict(entries=entries, pre=pre, post=ot.sdf_blocks().copy(), want=want, stats=stats, trace=t, at=at,
                        listed_ok=listed_ok, keys=key_set(ot.allocated()), inv=inv))
    ot.close()
    _runs[c.name] = out
    return out


ALL = [n for f in "abcdef" for n in TC.names(f)]


@pytest.mark.parametrize("name", ALL)
def test_rule_is_the_oracles_update(oracle, name):
    c = TC.case(oracle, name)
    for k, r in enumerate(oracle_run(oracle, c)):
        assert r["listed_ok"], (name, k)                                   # visible_entries is the oracle's compact list
        assert len(r["entries"]) >= 8 and r["stats"]["updated"] > 500, (name, k, len(r["entries"]), r["stats"])
        assert_same_voxels(r["want"], r["post"], c, f"frame {k}")
        print(f"{name} frame {k}: {len(r['entries'])} blocks listed, {r['stats']['updated']} voxels updated, "
              f"{r['stats']['untouched']} untouched")


def count_pairs(ok):
    """(cells where only the first voxel of the 16-byte pair changes, cells where only the second does)."""
    a, b = ok[:, 0::2], ok[:, 1::2]
    return int((a & ~b).sum()), int((~a & b).sum())


def value_counts(values, got, mask):
    """How many of got[mask] carry the bits of each of `values`."""
    g = bits(np.asarray(got, F))[mask]
    return {repr(float(F(v))): int((g == bits(np.array([v], F))[0]).sum()) for v in values}


def special_reads(c, t):
    """{special value: voxels inside the image that read a pixel holding it}."""
    ident = np.full((c.H, c.W), -1, np.int64)
    for i, pixels in c.special.items():
        for x, y in pixels:
            ident[y, x] = i
    got = ident[np.where(t["inb"], t["sy"], 0), np.where(t["inb"], t["sx"], 0)][t["inb"]]
    return {repr(c.depths[i]): int((got == i).sum()) for i in range(len(c.depths))}


def branches(c, t, pre_w):
    ok, inb = t["ok"], t["inb"]
    with np.errstate(invalid="ignore", over="ignore"):
        pos = inb & ~(t["depth"] <= F(0))
        cap = F(c.kw["integrationWeightMax"])
        total = pre_w + t["cw"]
        out = {"left of the image": int((t["sx"] < 0).sum()), "right of it": int((t["sx"] >= c.W).sum()),
               "above it": int((t["sy"] < 0).sum()), "below it": int((t["sy"] >= c.H).sum()),
               "depth <= 0": int((inb & (t["depth"] <= F(0))).sum()), "!(sdf > -trunc)": int((pos & ~(t["raw"] > -t["trunc"])).sum()),
               "clamped to +trunc": int((ok & (t["raw"] > t["trunc"])).sum()), "sdf < 0, kept": int((ok & (t["raw"] < F(0))).sum()),
               "below the cap": int((ok & (total < cap)).sum()), "at the cap": int((ok & (total == cap)).sum()),
               "above the cap": int((ok & (total > cap)).sum()), "cw clamped to 1": int((ok & (t["cw"] == F(1))).sum())}
    return out


@pytest.mark.parametrize("name", ALL)
def test_inputs_reach_what_they_aim_at(oracle, name):
    """The coverage conditions, on the reference alone.  (The lower clamp max(-trunc, sdf) cannot act on a voxel that passed
    sdf > -trunc; what is counted for it is the negative side being taken.)"""
    c = TC.case(oracle, name)
    runs = oracle_run(oracle, c)
    r = runs[0]
    t, ok = r["trace"], r["trace"]["ok"]
    pre_w, pre_s = r["pre"]["weight"][r["at"]], r["pre"]["sdf"][r["at"]]
    br = branches(c, t, pre_w)
    first, second = count_pairs(ok)
    print(f"{name}: {br}; cells with only voxel 0 changed {first}, only voxel 1 {second}")
    assert first > 0 and second > 0
    for side in ("left of the image", "right of it", "above it", "below it", "depth <= 0"):
        assert br[side] > 0 or c.sem == 0, (name, side)
    assert br["clamped to +trunc"] > 0 and br["sdf < 0, kept"] > 0, name
    if c.family in "abd":
        assert br["!(sdf > -trunc)"] > 0, name
    if c.family == "a":
        w, s = value_counts(c.weights, pre_w, ok), value_counts(c.sdfs, pre_s, ok)
        print(f"  stored weights updated: {w}\n  stored sdf updated: {s}")
        assert min(w.values()) > 0 and min(s.values()) > 0
        assert br["below the cap"] > 0 and br["above the cap"] > 0
        assert br["at the cap"] > 0                            # (0.25 - 0.1) + 0.1 == 0.25 in fp32; 2.0 + 1.0 == 3.0
        big = ok & (pre_w >= F(2.0 ** 24 if c.flags == 0 else 2.0 ** 30))
        assert big.sum() > 0 and np.array_equal((pre_w + t["cw"])[big], pre_w[big])          # ow + cw == ow
    if c.family in "bd":
        reads = special_reads(c, t)
        print(f"  special depths read inside the image: {reads}")
        assert min(reads.values()) > 0
        if c.flags & 2:
            assert br["cw clamped to 1"] > 0
        assert br["below the cap"] > 0
    if c.family == "b":
        if c.flags == 0:
            for tag, _, _ in TC.EXACT_TARGETS:
                assert len(c.marks[tag]) == 4
            print(f"  exact targets: { {k: len(v) for k, v in c.marks.items()} }")
        if c.flags & 1:
            moved = ok & (t["trunc"] != F(c.kw["truncation"]))
            assert moved.sum() > 100
    if c.family == "d":
        w, s = value_counts(c.weights, pre_w, ok), value_counts(c.sdfs, pre_s, ok)
        print(f"  rare stored weights updated: {w}\n  rare stored sdf updated: {s}")
        assert min(w.values()) > 0 and min(s.values()) > 0
        post = r["want"][r["at"]]
        nan = (np.isnan(post["sdf"]) | np.isnan(post["weight"])) & ok
        share = nan.sum() / ok.sum()
        print(f"  {int(nan.sum())} of {int(ok.sum())} updated voxels end as NaN: {share:.3f}")
        assert 0 < share < 0.5
    if c.family == "e":
        reads = special_reads(c, t)
        print(f"  special sensor values read inside the image: {reads}")
        assert min(reads.values()) > 0
        k = c.frames[0].sensor[1]
        assert k[6] != 0 and k[7] != 0
    if c.family == "c" and c.sem == 1:
        W, H = F(c.W), F(c.H)
        with np.errstate(invalid="ignore"):
            n = {"cz < 0": int((t["cz"] < 0).sum()), "cz == 0": int((t["cz"] == 0).sum()), "cz > 0": int((t["cz"] > 0).sum()),
                 "camera centre -> pixel (0, 0), updated": int((np.isnan(t["qx"]) & np.isnan(t["qy"]) & (t["sx"] == 0) & (t["sy"] == 0) & ok).sum()),
                 "qx in (-1, 0)": int(((t["qx"] > -1) & (t["qx"] < 0) & t["inb"]).sum()),
                 "qy in (-1, 0)": int(((t["qy"] > -1) & (t["qy"] < 0) & t["inb"]).sum()),
                 "qx == width": int((t["qx"] == W).sum()), "qy == height": int((t["qy"] == H).sum()),
                 "qx == width - 1": int(((t["qx"] == W - 1) & t["inb"]).sum()), "qy == height - 1": int(((t["qy"] == H - 1) & t["inb"]).sum()),
                 "qx in (width - 1, width)": int(((t["qx"] > W - 1) & (t["qx"] < W) & t["inb"]).sum()),
                 "qy in (height - 1, height)": int(((t["qy"] > H - 1) & (t["qy"] < H) & t["inb"]).sum()),
                 "updated with cz < 0": int((ok & (t["cz"] < 0)).sum())}
        print(f"  {n}")
        assert min(n.values()) > 0, n
    if c.family == "c" and c.sem == 0:
        # the index truncation: inverse pose on the voxel index, components that are whole, that lie in (-1, 0) (truncation and
        # floor differ) and that are negative and not whole
        e = r["entries"]
        lin = np.arange(512)
        base = e["pos"].astype(np.int64) * 8
        v = [(base[:, a:a + 1] + ((lin >> (3 * a)) & 7)[None, :]).astype(F) for a in range(3)]
        rr = np.stack(R._mat4_rows(r["inv"], *v))
        n = {"whole": int((rr == np.trunc(rr)).sum()), "in (-1, 0)": int(((rr > -1) & (rr < 0)).sum()),
             "negative, not whole": int(((rr < 0) & (rr != np.trunc(rr))).sum())}
        print(f"  index components: {n}")
        assert n["in (-1, 0)"] > 0 and n["negative, not whole"] > 0
        if "half-shift" in name:
            assert n["whole"] > 0 and int((np.abs(rr - np.trunc(rr)) == 0.5).sum()) > 0
    if c.family == "f":
        assert len(runs) == 3
        seen = set(c.blocks)
        for k, rk in enumerate(runs):
            new = rk["keys"] - seen
            shared = TC_keys(rk["entries"]) & (TC_keys(runs[k - 1]["entries"]) if k else set(c.blocks))
            print(f"  frame {k}: {len(new)} new blocks, {len(shared)} listed blocks shared with the frame before")
            assert len(shared) >= 4 and (k == 0 or len(new) > 0)
            seen = rk["keys"]
        assert len(seen) <= c.table["numVoxelBlocks"] - 8


def TC_keys(entries):
    return key_set(entries)


# ---- the removal's inputs (the oracle has no removal: the rule alone) ----------------------------------------------------
@pytest.mark.parametrize("name", TC.names("r"))
def test_removal_inputs_reach_the_floor(oracle, name):
    assert TC.names("r") == [c.name for c in TC.cases(oracle, "r")]
    c = TC.case(oracle, name)
    f = c.frames[0]
    inv = oracle.invert4x4(f.pose)
    e, vol = c.entries(), c.volume()
    p = c.rule_params
    listed = e[R.visible_entries(e, p, c.sem, c.proj, f.pose, inv, c.W, c.H)]
    assert len(listed) >= 24
    t = TC.trace(listed, p, c.sem, c.proj, inv, f.depth_source(), c.flags)
    out, stats = R.apply_frame(vol, listed, p, c.sem, c.proj, inv, f.pose, f.depth_source(), c.flags, -1)
    at = listed["ptr"].astype(np.int64)[:, None] + np.arange(512)[None, :]
    ow = vol["weight"][at]
    floor = TC.W_FLOOR[c.flags & 2]
    with np.errstate(invalid="ignore", over="ignore"):
        change = t["ok"] & (ow > 0)
        nw = ow - t["cw"]
        n = {"leaves the floor": int((change & (nw == floor)).sum()),
             "nearest above": int((change & (nw > floor) & (nw < floor * F(1.0001))).sum()),
             "nearest below": int((change & (nw < floor) & (nw > floor * F(0.9999))).sum())}
    print(f"{name}: {len(listed)} blocks, {stats}, {n}")
    assert stats["reset"] > 0 and stats["partial"] > 0 and stats["untouched"] > 0
    if name.startswith(("r-a", "r-d", "r-e")):
        assert n["nearest above"] > 0 and n["nearest below"] > 0
        if c.flags & 2:
            assert n["leaves the floor"] > 0           # 1.5 - 1; its fp32 neighbours leave the nearest values on either side
    if not nonfinite(c):
        assert not np.isnan(out["sdf"]).any() and not np.isnan(out["weight"]).any()
    else:
        upd = change
        nan = (np.isnan(out["sdf"][at]) | np.isnan(out["weight"][at])) & upd
        print(f"  {int(nan.sum())} of {int(upd.sum())} changed voxels end as NaN")
        assert nan.sum() < 0.5 * upd.sum()


# ---- the rule over several frames and cameras ------------------------------------------------------------------------------
def expected_by_rule(oracle, c, params, pre_vox, post_table, steps, keysets, sign=+1):
    """The volume by the rule from `pre_vox`: steps[b] is the list of Frames (cameras, in camera order) of frame b, each
    applied over its own visible set -- visible_entries of the table as it was after frame b's allocation: `post_table` (the
    table after all frames; a block keeps its slot and its heap block once it has them) with the entries whose key is not in
    keysets[b] (the oracle's allocated keys after frame b) taken out.  A block new in a frame starts from the zeros of
    `pre_vox`.  Returns (volume, voxels updated)."""
    vox, updated = pre_vox, 0
    for cams, keys in zip(steps, keysets):
        tab = post_table.copy()
        absent = np.array([tuple(p) not in keys for p in tab["pos"].tolist()], bool) & (tab["ptr"] != -1)
        tab["ptr"][absent] = -1
        for f in cams:
            inv = oracle.invert4x4(f.pose)
            listed = tab[R.visible_entries(tab, params, c.sem, c.proj, f.pose, inv, c.W, c.H)]
            vox, stats = R.apply_frame(vox, listed, params, c.sem, c.proj, inv, f.pose, f.depth_source(), c.flags, sign)
            updated += stats["updated"] + stats["reset"] + stats["partial"]
    return vox, updated


_multi = {}
MULTI = [("a-cap025-48x32", 1), ("a-cap3-both-flags-48x32", 2), ("b-flags0-48x32", 1), ("b-flags3-48x32", 2), ("e-flags0-48x32", 1),
         ("e-flags3-48x32", 2), ("f-flags0-48x32", 2), ("f-flags3-33x17", 1)]
MULTI_SIZE = (320, 240)


def oracle_multi(oracle, name, batch):
    """(case, keysets): the two-camera frames of tsdf_cases.multi_camera on ONE oracle table (reference_multi_camera_frame's
    order: one lock epoch, every camera's allocation, then list + update camera by camera), checked against the rule."""
    from voxelhashing_demo_amd import dist as vdist
    if (name, batch) in _multi:
        return _multi[(name, batch)]
    t = TC.multi_camera(oracle, TC.case(oracle, name), *MULTI_SIZE, batch)
    ot = load_oracle(oracle, t)
    pre = ot.sdf_blocks().copy()
    keysets = []
    for cams in t.steps:
        vdist.reference_multi_camera_frame(ot, [f.pose for f in cams], [f.verts for f in cams])
        keysets.append(key_set(ot.allocated()))
    assert len(keysets[-1]) <= t.table["numVoxelBlocks"] - 8, len(keysets[-1])
    want, updated = expected_by_rule(oracle, t, ot.params, pre, ot.hash_table().copy(), t.steps, keysets)
    assert_same_voxels(want, ot.sdf_blocks(), t)
    assert updated > 1000
    t.updated, t.new_blocks = updated, len(keysets[-1]) - len(t.blocks)
    ot.close()
    _multi[(name, batch)] = (t, keysets)
    return t, keysets


@pytest.mark.parametrize("name,batch", MULTI)
def test_rule_camera_by_camera_is_the_oracles_multi_camera_frame(oracle, name, batch):
    t, keysets = oracle_multi(oracle, name, batch)
    print(f"{t.name}: {t.updated} voxel updates over {len(t.steps)} frames of two cameras, {t.new_blocks} new blocks")
