"""Band allocation on crafted pixels (tests/band_cases.py), every frame form of the HIP path against the oracle slot for slot,
and the GPU's own keys against the rule restated exactly (tests/band_ref.py): block corners, edges and faces, axis-parallel
and zero-length segments, the 62-step cap, special values in the normal, quotients one ulp from a rounding tie on both sides of
the range gates of the hoisted divisions, and images whose lanes differ as much as lanes can.
tests/test_band_ref_cpu.py pins the reference and the inputs against the oracle."""
import pytest

import band_cases as BC
from test_band_ref_cpu import (MAX_FRAMES, bounds_of, converge, decode_records, exact_pixel_keys, in_frustum, make_oracle,
                               oracle_pixel_keys, sensor_table_image, wave_collapse)
from test_gpu_gc import VARIANTS
from test_gpu_overflow import pair
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu
FORMS = list(VARIANTS) + ["pipelined-batches-of-3"]
SENSOR = "c-sensor"
NAMES = [i.name for i in BC.all_images()] + [SENSOR]
_images, _oracles, _refs = {}, {}, {}


def image(oracle, name):
    if not _images:
        _images.update({i.name: i for i in BC.all_images()})
    if name == SENSOR and name not in _images:
        s = BC.sensor_image()
        _images[name] = sensor_table_image(oracle, s)
        _images[name].depth, _images[name].kinv = s[0], s[1]
    return _images[name]


def reference(oracle, img):
    """Once per image: the oracle's keys per pixel, the restated rule's keys per pixel (exact families) or bounds (family b),
    all after the oracle's frustum test."""
    if img.name not in _refs:
        ot = make_oracle(oracle, img)
        r = {"oracle": oracle_pixel_keys(oracle, img)}
        if img.family == "b":
            r["bounds"] = {}
            for xy in img.pixels:
                must, may = bounds_of(img, xy)
                r["bounds"][xy] = ({k for k in must if ot.block_in_frustum(k)}, {k for k in may if ot.block_in_frustum(k)})
        else:
            r["exact"] = {xy: in_frustum(ot, exact_pixel_keys(img, xy)) for xy in img.pixels}
            r["exact"] = {xy: v for xy, v in r["exact"].items() if v}
        ot.close()
        _refs[img.name] = r
    return _refs[img.name]


def oracle_after(oracle, img, frames=None):
    """The oracle's table after `frames` frames of the image (None: as many as it takes to stop growing); kept, never changed."""
    if (img.name, None) not in _oracles:
        ot = make_oracle(oracle, img)
        n = converge(ot, img)
        assert ot.last_stats["heap_exhausted"] == 0
        _oracles[(img.name, None)] = _oracles[(img.name, n)] = (ot, n)
    if frames is None or (img.name, frames) in _oracles:
        return _oracles[(img.name, frames)]
    ot = make_oracle(oracle, img)
    for _ in range(frames):
        ot.integrate(img.T, img.verts, img.normals)
    _oracles[(img.name, frames)] = (ot, frames)
    return ot, frames


def gpu_table(oracle, vh, img, variant):
    spare, gt = pair(oracle, vh, variant, img.W, img.H, img.sem, overflow=False, voxelSize=img.vs, **BC.TABLE)
    spare.close()
    gt.set_projection(img.proj)
    gt.set_alloc_band(img.band)
    gt.set_option("band_mode", img.mode)
    return gt


def check_keys_of_model(oracle, img, keys):
    """The allocated set against the restated rule directly: equal (exact families), between the unions of MUST and MAY (b)."""
    ref = reference(oracle, img)
    if img.family == "b":
        must = set().union(*[m for m, _ in ref["bounds"].values()])
        may = set().union(*[m for _, m in ref["bounds"].values()])
        assert must <= keys <= may, (sorted(must - keys)[:5], sorted(keys - may)[:5])
    else:
        assert keys == {key for v in ref["exact"].values() for _, key in v}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_crafted_frames_equal_the_oracle(oracle, vh, torch_cuda, name, form):
    torch = torch_cuda
    img = image(oracle, name)
    ot, n = oracle_after(oracle, img)
    pipelined = form not in VARIANTS
    gt = gpu_table(oracle, vh, img, "fused-ballot-walk" if pipelined else form)
    dv = torch.from_numpy(img.verts).cuda()
    dn = None if img.normals is None else torch.from_numpy(img.normals).cuda()
    dd = torch.from_numpy(img.depth).cuda() if name == SENSOR else None
    totals = []
    if pipelined:
        gt.set_option("pipeline", 1)
        n = 3 * ((n + 2) // 3)
        ot, _ = oracle_after(oracle, img, n)
        for _ in range(n // 3):
            if dd is not None:
                gt.integrate_depth_batch([img.T] * 3, [dd] * 3, img.kinv)
            else:
                gt.integrate_batch([img.T] * 3, [dv] * 3, None if dn is None else [dn] * 3)
            totals.append(gt.counters()["allocated_total"])
        assert totals[-1] == len(ot.allocated())           # (the last batch holds the frame at which the oracle stopped growing)
    else:
        for _ in range(MAX_FRAMES):
            if dd is not None:
                gt.integrate_depth(img.T, dd, img.kinv)
            else:
                gt.integrate(img.T, dv, dn)
            totals.append(gt.counters()["allocated_total"])
            if len(totals) > 1 and totals[-1] == totals[-2]:
                break
        assert len(totals) == n, f"the GPU's table stopped growing after {len(totals)} frames, the oracle's after {n}"
    gt.synchronize()
    assert gt.counters()["heap_exhausted"] == 0 and totals[-1] > 0
    _compare(ot, gt)
    check_keys_of_model(oracle, img, set(map(tuple, gt.allocated()["pos"].tolist())))
    gt.close()


@pytest.mark.parametrize("name", [i.name for i in BC.all_images() if i.mode != BC.NORMAL_DDA])
def test_crafted_key_records(oracle, vh, torch_cuda, name):
    """vh_generate_keys: per pixel the records are the oracle's (after its frustum test and the waves' documented collapse of
    equal keys), and they are what the restated rule gives."""
    torch = torch_cuda
    img = image(oracle, name)
    ref = reference(oracle, img)
    gt = gpu_table(oracle, vh, img, "fused-ballot-walk")
    gt.set_pose(img.T)
    cap = img.W * img.H * 32 + 1
    bins = torch.zeros((1, cap, 4), dtype=torch.int32, device="cuda")
    gt.generate_keys(torch.from_numpy(img.verts).cuda(), 0, 1, bins, cap)
    gt.synchronize()
    got = bins.cpu().numpy()
    count = int(got[0, 0, 0])
    assert 0 < count < cap and gt.counters()["bin_overflow"] == 0
    mine = decode_records(got[0, 1:count + 1], img.W)
    want = wave_collapse(ref["oracle"], img.W, img.H)
    assert set(mine) == set(want)
    for xy in want:
        assert mine[xy] == want[xy], (name, xy, img.pixels.get(xy))
    if img.family == "b":
        for xy, (must, may) in ref["bounds"].items():
            keys = {key for _, key in mine.get(xy, [])}
            assert must <= keys <= may, (name, xy, img.pixels[xy])
    else:
        assert mine == wave_collapse(ref["exact"], img.W, img.H)
    gt.close()
