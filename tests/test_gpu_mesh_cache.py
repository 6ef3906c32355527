"""vh_changes and vh_extract_mesh_blocks tied together by MeshCache, on random sequences of every model-changing call (the
generator of tests/lifecycle_cases.py, cut off by tests/mesh_cache_cases.py; then one vh_remove_components): after every step
and one MeshCache.update(), the cache holds exactly the allocated keys and every chunk is the fresh per-block extraction, bit
for bit -- without normals (halo MESH) and with them (halo NORMALS).  tests/test_changes_ref_cpu.py shows on the shadow model
that the sequences have steps that list fewer blocks than the model holds; here at least one update must re-extract fewer."""
import numpy as np
import pytest

import lifecycle_cases as LC
import lifecycle_ref as LR
import merge_color_cases as CC
import mesh_cache_cases as MC
from test_gpu_lifecycle import run_call, source_table
from voxelhashing_demo_amd.meshing import MeshCache

pytestmark = pytest.mark.gpu
U = np.uint32


def check(gt, cache, normals):
    """One update, then the cache against a fresh extraction of every allocated block."""
    stats = cache.update()
    keys = [tuple(k) for k in gt.allocated()["pos"].tolist()]
    assert set(cache.blocks) == set(keys) and len(set(keys)) == len(keys)
    pos, nrm, first = gt.extract_mesh_blocks(np.array(keys, np.int32).reshape(-1, 3), normals=normals)
    first = first.astype(np.int64)
    for j, k in enumerate(keys):
        a, b = int(first[j]), int(first[j + 1])
        got = cache.blocks[k]
        if normals:
            assert got[0].shape == pos[a:b].shape and np.array_equal(got[0].view(U), pos[a:b].view(U)), k
            assert np.array_equal(got[1].view(U), nrm[a:b].view(U)), k
        else:
            assert got.shape == pos[a:b].shape and np.array_equal(got.view(U), pos[a:b].view(U)), k
    assert stats["extracted"] == stats["changed"] <= len(keys) and stats["triangles"] <= len(pos)
    return stats, len(keys), len(pos)


@pytest.mark.parametrize("normals", [False, True], ids=["halo mesh", "halo normals"])
@pytest.mark.parametrize("seed", MC.SEEDS)
def test_the_cache_follows_every_call(oracle, vh, torch_cuda, tmp_path, seed, normals):
    torch = torch_cuda
    seq = LC.Sequence(oracle, MC.VARIANT, MC.SEM, seed)
    kw, overflow = LR.VARIANTS[MC.VARIANT]
    gt = CC.table(vh, kw, MC.SEM)
    src = source_table(vh, seq)
    cache = MeshCache(gt, normals=normals)
    partial, ops, removed, most = [], [], 0, 0
    for n, step in MC.changing_steps(seq):
        if not MC.changes_model(step):
            if step["op"] in LC.OPTIONS:
                run_call(torch, gt, src, seq, step, tmp_path)
            continue
        run_call(torch, gt, src, seq, step, tmp_path)          # (a frame left pending is launched by the update's vh_changes)
        try:
            stats, blocks, triangles = check(gt, cache, normals)
        except AssertionError as e:
            raise AssertionError(f"seed {seed}, step {n} {step['op']} after {ops}: {e}") from e
        ops.append(step["op"])
        removed += stats["removed"]
        most = max(most, triangles)
        if stats["extracted"] < blocks:
            partial.append((n, step["op"], stats["extracted"], blocks))
    # the one call the generator does not draw: small pieces out of the volume, emptied blocks freed
    gt.remove_components(40)
    stats, blocks, triangles = check(gt, cache, normals)
    print(f"seed {seed}: steps={len(ops)} partial={partial} removed={removed} remove_components: {stats} of {blocks} blocks")
    assert stats["extracted"] < blocks
    assert len(partial) >= 3 and removed > 0 and most > 100
    whole = cache.triangles()
    assert len(whole[0] if normals else whole) == triangles
    # nothing pending: an update right after lists nothing
    assert cache.update() == {"changed": 0, "removed": 0, "extracted": 0, "triangles": 0}
    gt.close()
    src.close()
    seq.close()
