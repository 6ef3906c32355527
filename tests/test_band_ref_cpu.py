"""Band allocation on crafted pixels, CPU side: pins tests/band_ref.py (the rule, restated exactly) and tests/band_cases.py (the
inputs and the properties their generator promises) against the oracle.  tests/test_gpu_band_crafted.py holds the HIP path to
both.  Every family prints its counts and asserts that they are not vacuous."""
import numpy as np
import pytest

import band_cases as BC
import band_ref as BR

F = np.float32
MAX_FRAMES = 70


# ---------------------------------------------------------------------------
# shared with the GPU tests
# ---------------------------------------------------------------------------
def make_oracle(oracle, img):
    ot = oracle.OracleTable(img.params(oracle), img.W, img.H, img.sem)
    ot.set_projection(img.proj)
    ot.set_alloc_band(img.band, img.mode)
    ot.set_pose(img.T)
    if img.normals is not None:
        ot.set_normals(img.normals)
    return ot


def decode_records(recs, W):
    """{(x, y): [(k, key)]} (k ascending) from key records {x, y, z, camera << 27 | launch rank << 6 | sample}."""
    tiles_x = (W + 15) // 16
    out = {}
    for kx, ky, kz, r in np.asarray(recs).tolist():
        r &= 0xffffffff
        k, lr = r & 63, (r >> 6) & ((1 << 21) - 1)
        tile, t = lr >> 8, lr & 255
        xy = ((tile % tiles_x) * 16 + (t & 15), (tile // tiles_x) * 16 + (t >> 4))
        out.setdefault(xy, []).append((k, (kx, ky, kz)))
    for v in out.values():
        v.sort()
    return out


def oracle_pixel_keys(oracle, img, verts=None):
    """{(x, y): [(k, key)]}: every key of every pixel that passes the oracle's frustum test, nothing collapsed.  generate_keys
    collapses runs of equal keys along an image row, so the image is handed over in two halves, even and odd columns, each with
    the other's pixels invalid."""
    verts = img.verts if verts is None else verts
    ot = make_oracle(oracle, img)
    out = {}
    for parity in (0, 1):
        v = verts.copy()
        v[:, (1 - parity)::2] = 0
        if not v[..., 2].any():
            continue
        bins, _ = ot.generate_keys(v, 0, 1, img.W * img.H * 32 + 1)
        out.update(decode_records(bins[0, 1:bins[0, 0, 0] + 1], img.W))
    ot.close()
    return out


def wave_collapse(pix, W, H):
    """What the claim phase's waves keep of `pix` (documented above sample_key in csrc/vh_alloc.hip): a lane drops sample k when
    its own previous sample, sample k of the lane to its left (same 16-pixel tile row) or sample k of the lane above (same
    16x4 wave) has the same key."""
    have = {xy: set(v) for xy, v in pix.items()}
    out = {}
    for (x, y), lst in pix.items():
        kept, prev = [], None
        for k, key in lst:
            dup = key == prev
            prev = key
            if x % 16 and (k, key) in have.get((x - 1, y), ()):
                dup = True
            if (y % 16) % 4 and (k, key) in have.get((x, y - 1), ()):
                dup = True
            if not dup:
                kept.append((k, key))
        if kept:
            out[(x, y)] = kept
    return out


def exact_pixel_keys(img, xy, info=None):
    """[(k, key)] of the pixel by the restated rule: band_ref.walk_exact on the fp32 end points, or band_ref.ray_samples."""
    if img.mode == BC.RAY:
        return BR.ray_samples(img.vertex(xy), img.vs, img.band, img.T)
    A, B = img.reference_ends(xy)
    if B is None:
        return [(0, BR.world2block_f32(A, img.vs))]
    return list(enumerate(BR.walk_exact(A, B, img.vs, info=info)))


def in_frustum(ot, keys):
    return [(k, key) for k, key in keys if ot.block_in_frustum(key)]


def converge(ot, img, frames=MAX_FRAMES):
    """Frames of the image until the table stops growing (one insertion per bucket and frame); returns how many were fused."""
    prev = -1
    for f in range(frames):
        ot.integrate(img.T, img.verts, img.normals)
        n = len(ot.allocated())
        if n == prev:
            return f + 1
        prev = n
    raise AssertionError(f"{img.name}: still growing after {frames} frames")


def bounds_of(img, xy):
    """(MUST, MAY) of a general pixel; both {block} for a pixel that demands its surface block only."""
    A, B = img.reference_ends(xy)
    if B is None:
        key = BR.world2block_f32(A, img.vs)
        return {key}, {key}
    assert all(np.isfinite(float(c)) for c in list(A) + list(B)), (img.name, xy)
    return BR.must_may(A, B, img.vs, BR.eps_voxels(A, B, img.vs, extra=img.vertex(xy)[:3]))


# ---------------------------------------------------------------------------
# a: exact cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("img", BC.images("a") + BC.images("d"), ids=lambda i: i.name)
def test_exact_walks_equal_the_oracle_in_keys_and_order(oracle, img):
    want_keys, ties, capped, pixels = 0, 0, 0, 0
    got = oracle_pixel_keys(oracle, img)
    ot = make_oracle(oracle, img)
    union = set()
    for xy in img.pixels:
        info = {}
        want = in_frustum(ot, exact_pixel_keys(img, xy, info))
        assert got.get(xy, []) == want, (img.name, xy, img.pixels[xy])
        ties += info.get("ties", 0)
        capped += bool(info.get("capped"))
        want_keys += len(want)
        pixels += 1
        union |= {key for _, key in want}
    print(f"{img.name}: {pixels} pixels, {want_keys} keys, {len(union)} blocks, {ties} tie steps, {capped} capped walks")
    assert want_keys >= pixels and len(union) < BC.TABLE["numVoxelBlocks"]
    if img.mode == BC.NORMAL_DDA:                      # ... and the frames' own path: the allocated set once it stops growing
        converge(ot, img)
        assert set(map(tuple, ot.allocated()["pos"].tolist())) == union
        assert ot.last_stats["heap_exhausted"] == 0
    ot.close()


def test_exact_family_is_not_vacuous():
    tags, ties, capped, sixty_two = set(), 0, 0, 0
    for img in BC.images("a"):
        for xy, tag in img.pixels.items():
            info = {}
            keys = exact_pixel_keys(img, xy, info)
            tags.add(tag.split(" ")[0])
            ties += info.get("ties", 0)
            capped += bool(info.get("capped"))
            sixty_two += len(keys) == 63 and not info.get("capped")
    print(f"family a: tags {sorted(tags)}, {ties} tie steps, {capped} capped walks, {sixty_two} walks of exactly 62 steps")
    assert {"corner", "edge", "along-edge", "face-start", "in-face", "axis", "zero", "floor", "cap", "cap-62", "cap-63",
            "z-b>0", "z-b=0", "z-b<0"} <= tags
    assert ties >= 300 and capped >= 9 and sixty_two >= 4
    ws = {float(img.vertex(xy)[3]) for img in BC.images("a") for xy in img.pixels}
    assert ws == {0.0, 1.0, 2.0}
    spread = next(i for i in BC.images("a") if i.name.endswith("spread"))          # no two pixels of it share a block
    keys = [key for xy in spread.pixels for _, key in exact_pixel_keys(spread, xy)]
    assert len(keys) == len(set(keys)) > 800


def test_tie_order_of_the_rule():
    """Known answers, by hand from the documented order (x only if strictly smallest, then z if smaller than y, else y)."""
    vs = BC.VS6
    assert BR.walk_exact([3.5 * vs] * 3, [11.5 * vs] * 3, vs) == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 1)]
    assert BR.walk_exact([3.5 * vs, 3.5 * vs, 2 * vs], [11.5 * vs, 11.5 * vs, 2 * vs], vs) == [(0, 0, 0), (0, 1, 0), (1, 1, 0)]
    assert BR.walk_exact([3.5 * vs, 2 * vs, 3.5 * vs], [11.5 * vs, 2 * vs, 11.5 * vs], vs) == [(0, 0, 0), (0, 0, 1), (1, 0, 1)]
    assert BR.walk_exact([2 * vs, 3.5 * vs, 3.5 * vs], [2 * vs, 11.5 * vs, 11.5 * vs], vs) == [(0, 0, 0), (0, 1, 0), (0, 1, 1)]
    # the first boundary is 8k - 0.5: a segment from voxel 7 to voxel 7.75 changes block, one from 7.5 to 8.25 does not
    assert BR.walk_exact([7 * vs, 0, 0], [7.75 * vs, 0, 0], vs) == [(0, 0, 0), (1, 0, 0)]
    assert BR.walk_exact([7.5 * vs, 0, 0], [8.25 * vs, 0, 0], vs) == [(1, 0, 0)]
    assert BR.walk_exact([-0.5 * vs, 0, 0], [-0.25 * vs, 0, 0], vs) == [(-1, 0, 0), (0, 0, 0)]     # half away from zero


# ---------------------------------------------------------------------------
# b: general cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("img", BC.images("b"), ids=lambda i: i.name)
def test_general_walks_lie_between_must_and_may(oracle, img):
    got = oracle_pixel_keys(oracle, img)
    ot = make_oracle(oracle, img)
    n_must = n_may = n_got = 0
    for xy in img.pixels:
        must, may = bounds_of(img, xy)
        assert must <= may and len(may) <= BR.MAX_STEPS, (img.name, xy)          # (no general case runs into the cap)
        seen = got.get(xy, [])
        keys = {key for _, key in seen}
        vis_must, vis_may = {k for k in must if ot.block_in_frustum(k)}, {k for k in may if ot.block_in_frustum(k)}
        assert vis_must <= keys <= vis_may, (img.name, xy, img.pixels[xy], sorted(vis_must - keys), sorted(keys - vis_may))
        for (k0, a), (k1, b) in zip(seen, seen[1:]):
            if k1 == k0 + 1:
                assert sorted(abs(a[i] - b[i]) for i in range(3)) == [0, 0, 1], (img.name, xy)
        n_must, n_may, n_got = n_must + len(must), n_may + len(may), n_got + len(keys)
    share = (n_may - n_must) / n_may
    print(f"{img.name}: {len(img.pixels)} pixels, {n_got} keys in the frustum, MUST {n_must}, MAY {n_may}, undecided {share:.4%}")
    assert n_got >= len(img.pixels) // 2
    if img.name.startswith("b-random"):
        assert share <= 0.05 and n_got > 2 * len(img.pixels)
    ot.close()


def test_general_family_is_not_vacuous():
    n_must = n_may = 0
    for img in BC.images("b"):
        if img.name.startswith("b-random"):
            assert 0.005 <= img.vs <= 0.05 and 1 <= img.band / img.vs <= 40
            for xy in img.pixels:
                must, may = bounds_of(img, xy)
                n_must, n_may = n_must + len(must), n_may + len(may)
    print(f"family b, seeded random cases: MUST {n_must}, MAY {n_may}, undecided {(n_may - n_must) / n_may:.4%}")
    assert n_may > 3000 and (n_may - n_must) <= 0.05 * n_may
    tags = {t for img in BC.images("b") for t in img.pixels.values()}
    assert {"dir.y denormal", "dir.y = 2^-120: tdelta overflows", "-0.0", "NaN x", "NaN y", "NaN z", "zero normal", "length 3",
            "z denormal", "z negative"} <= tags


# ---------------------------------------------------------------------------
# c: division cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("img", BC.images("c"), ids=lambda i: i.name)
def test_ray_samples_equal_the_oracle(oracle, img):
    got = oracle_pixel_keys(oracle, img)
    ot = make_oracle(oracle, img)
    n = 0
    for xy in img.pixels:
        want = in_frustum(ot, exact_pixel_keys(img, xy))
        assert got.get(xy, []) == want, (img.name, xy, img.pixels[xy])
        n += len(want)
    print(f"{img.name}: {len(img.pixels)} pixels, {n} keys, half = {BR.ray_half(img.vs, img.band)}")
    assert n >= len(img.pixels)
    ot.close()


def test_division_cases_keep_what_their_generator_promises():
    direct = scaled = 0
    paths = {"scale": set(), "vs": set()}
    by_image = {}
    for img in BC.images("c"):
        mine = {"scale": set(), "vs": set()}
        for xy in img.pixels:
            x, y, z, w = [F(c) for c in img.vertex(xy)]
            if img.kind[xy] == "direct":                 # each coordinate's quotient: one ulp either way changes the block
                assert all(BC.ulp_sensitive(F(c / F(img.vs))) for c in (x, y, z)), (img.name, xy)
                direct += 1
            elif img.kind[xy] == "scaled":
                k, half = img.sensitive_sample[xy], BR.ray_half(img.vs, img.band)
                s = F(z + F(F(F(k) - F(half)) * F(F(4) * F(img.vs))))
                sc = F(s / z)
                assert s > 0 and BC.ulp_sensitive(F(s / F(img.vs)))
                for c in (x, y):
                    q = F(F(c * sc) / F(img.vs))
                    assert BC.ulp_sensitive(q)
                    moved = [BC._block1(F(F(c * o) / F(img.vs))) for o in (np.nextafter(sc, F(0)), np.nextafter(sc, F(np.inf)))]
                    assert any(m != BC._block1(q) for m in moved), (img.name, xy)
                scaled += 1
            p = BC.division_paths(img, xy)
            for d in mine:
                mine[d] |= p[d]
        by_image[img.name] = mine
        for d in paths:
            paths[d] |= mine[d]
    print(f"family c: {direct} direct cases, {scaled} scaled cases, paths {paths}")
    print("\n".join(f"  {k}: {v}" for k, v in by_image.items()))
    assert direct >= 200 and scaled >= 200
    assert paths == {"scale": {"fast", "plain"}, "vs": {"fast", "plain"}}
    # the gates, each from both sides
    assert by_image["c-gate-vs-lo-in"]["vs"] == {"fast"} and by_image["c-gate-vs-lo-out"]["vs"] == {"plain"}
    assert by_image["c-gate-vs-hi-in"]["vs"] == {"fast"} and by_image["c-gate-vs-hi-out"]["vs"] == {"plain"}
    assert by_image["c-gate-s-lo"]["scale"] == {"fast", "plain"} and by_image["c-gate-s-hi"]["scale"] == {"fast", "plain"}
    zg = BC.images("c")[len(BC.DIVISORS)]
    assert zg.name == "c-gate-z-g"
    per_pixel = {zg.pixels[xy]: BC.division_paths(zg, xy) for xy in zg.pixels}
    up = float(np.nextafter(F(2.0 ** 40), F(np.inf)))
    assert per_pixel[f"z={(2.0 ** 40).hex()}"]["scale"] == {"fast"} and per_pixel[f"z={up.hex()}"]["scale"] == {"plain"}
    dn = float(np.nextafter(F(2.0 ** -40), F(0)))
    assert per_pixel[f"z={(2.0 ** -40).hex()}"]["scale"] == {"fast"} and per_pixel[f"z={dn.hex()}"]["scale"] == {"plain"}
    assert "fast" in per_pixel[f"g={(2.0 ** 50).hex()}"]["vs"] and "plain" in per_pixel[f"g={(0.0).hex()}"]["vs"]
    assert any(BR.ray_half(i.vs, i.band) == 31 for i in BC.images("c"))
    assert {float(F(d)) for d in BC.DIVISORS} <= {i.vs for i in BC.images("c")}


@pytest.fixture(scope="module")
def sensor():
    return BC.sensor_image()


def sensor_table_image(oracle, sensor):
    """The sensor case as an Image: the vertex map preProcess makes of the depth image."""
    depth, kinv, found = sensor
    img = BC.Image("c-sensor", 48, 32, BC.RAY, 0.02, 0.1, BC.I4, BC.ALL_PASS, "c")
    img.verts = oracle.preprocess(depth, kinv)[0]
    img.pixels = {xy: "sensor" for xy in found}
    return img


def test_sensor_depths_next_to_a_tie(oracle, sensor):
    depth, kinv, found = sensor
    img = sensor_table_image(oracle, sensor)
    hits = 0
    for (x, y), n in found.items():
        v = img.verts[y, x]
        assert v[2] != 0
        mine = sum(BC.ulp_sensitive(F(F(c) / F(img.vs))) for c in v[:3])
        assert mine == n                                  # (the search's arithmetic is preProcess's, bit for bit)
        hits += mine
    got = oracle_pixel_keys(oracle, img)
    ot = make_oracle(oracle, img)
    for xy in img.pixels:
        assert got.get(xy, []) == in_frustum(ot, exact_pixel_keys(img, xy)), xy
    print(f"sensor path: {len(found)} pixels with {hits} coordinates next to a tie")
    assert len(found) >= 100 and hits >= len(found)
    ot.close()
