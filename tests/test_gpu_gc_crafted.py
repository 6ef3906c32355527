"""vh_delete_blocks and vh_garbage_collect on crafted buckets, chains and voxels (tests/gc_cases.py): the oracle's state is loaded
slot for slot as a snapshot, the downloaded pre-state must equal it bit for bit, the same call is made on both sides, and then

  - the table equals the oracle's entry for entry (pos, offset AND ptr), every voxel of the volume bit for bit;
  - the GPU's own post-state passes the state check written from the definition (gc_cases.check_after);
  - the occupancy index still knows every bucket that holds something: set_pose + flatten list the oracle's compact set with
    the indexed walk (flatten_variant 4) and with the reference's (3);
  - the table goes on: stream_in places every deleted key again and the next flatten finds them.

tests/test_gc_cases_cpu.py pins the cases and the state check to the oracle without a GPU.  Comparisons are exact."""
import functools
import time

import numpy as np
import pytest

import gc_cases as GC
import mesh_models as mm
from test_gc_cases_cpu import CHAINS, MASKS, PLAIN, case
from test_gpu_deintegrate import dev, snapshot
from test_gpu_tsdf_crafted import FORMS, PLACED

pytestmark = pytest.mark.gpu
U = np.uint32


@functools.lru_cache(maxsize=None)
def _oracle_run(name, threshold, big):
    """(case, pre, post, freed, compact set at the case's pose after the call) on the oracle, once a case."""
    import oracle
    if name.startswith("V"):
        c = GC.v_case(oracle, threshold, big)
    elif name.startswith("W"):
        c = GC.w_case(int(name.split("-")[2]), "shard" in name)
    else:
        c = case(name)
    ot = GC.load_oracle(oracle, c)
    pre = GC.state_of(ot)
    freed = GC.oracle_call(c, ot)
    post = GC.state_of(ot)
    ot.set_pose(c.pose)
    ot.flatten()
    listed = set(map(tuple, ot.compact()["pos"].tolist()))
    ot.close()
    return c, pre, post, freed, listed


def oracle_run(name, threshold="T", big=False):
    return _oracle_run(name, threshold, big)


def loaded_table(vh, c, pre, tmp_path, **options):
    """A context of the case that holds the oracle's pre-state slot for slot; the downloaded state is checked against it."""
    gt = vh.SDFHashtable(c.params(vh), c.W, c.H, c.sem, bucket_range=c.bucket_range)
    gt.set_projection(c.proj())
    if c.overflow:
        gt.set_option("overflow_list", 1)
    for k, v in options.items():
        gt.set_option(k, v)
    mm.load_state(gt, pre["table"], pre["heap"], pre["heap_counter"], pre["vox"], tmp_path)
    got = snapshot(gt)
    assert np.array_equal(got["table"], pre["table"]) and got["heap_counter"] == pre["heap_counter"]
    assert np.array_equal(got["vox"].view(U), pre["vox"].view(U))
    n = pre["heap_counter"] + 1
    assert np.array_equal(got["heap"][:n], pre["heap"][:n])
    return gt, got


def same_as_oracle(c, gt, mine, want, doomed, freed, counters_before):
    """Table, voxels and counters after the call against the oracle's; the state check on the GPU's own states."""
    got = snapshot(gt)
    for f in ("pos", "offset", "ptr"):
        assert np.array_equal(got["table"][f], want["table"][f]), f"{c.name}: {f} differs from the oracle's"
    assert np.array_equal(got["vox"].view(U), want["vox"].view(U)), f"{c.name}: voxels differ from the oracle's"
    assert got["heap_counter"] == want["heap_counter"]
    k = gt.counters()
    assert k["last_freed"] == freed and k["occupied"] == 0
    n = GC.check_after(mine, got, doomed, c.shape, (k["last_freed"], counters_before["freed_total"], k["freed_total"]))
    assert n == freed == len(doomed)
    return got


def index_and_way_back(c, gt, listed, back, pre):
    """The occupancy index (walk 4) and the reference's walk (3) list the oracle's compact set; then the deleted keys come back."""
    survivors = set(c.insert) - set(k for call in back for k in call)
    assert listed == survivors, "the case's pose does not see every survivor"
    for walk in (4, 3):
        gt.set_option("flatten_variant", walk)
        gt.set_pose(c.pose)
        assert gt.flatten() == len(listed), f"{c.name}: walk {walk}"
        assert set(map(tuple, gt.compact()["pos"].tolist())) == listed, f"{c.name}: walk {walk}"
    where = {tuple(e["pos"].tolist()): int(e["ptr"]) for e in pre["table"][pre["table"]["ptr"] != -1]}
    for call in back:
        vox = np.stack([pre["vox"][where[k]:where[k] + 512] for k in call])
        st = gt.stream_in({"keys": np.array(call, np.int32), "voxels": vox})
        assert st["placed"] == len(call) and (st["status"] == PLACED).all(), f"{c.name}: {st}"
    gt.set_option("flatten_variant", 4)
    gt.set_pose(c.pose)
    assert gt.flatten() == len(c.insert)
    assert set(map(tuple, gt.compact()["pos"].tolist())) == set(c.insert)
    tab, vol = gt.hash_table(), gt.sdf_blocks()
    for e in tab[tab["ptr"] != -1][::7]:                                   # ... with their voxels
        k, p = tuple(e["pos"].tolist()), int(e["ptr"])
        assert np.array_equal(vol[p:p + 512].view(U), pre["vox"][where[k]:where[k] + 512].view(U))


# ---- 1. delete_blocks: plain buckets, one chain, interleaved chains ----------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN + CHAINS)
def test_delete_blocks(vh, torch_cuda, tmp_path, name):
    c, pre, post, freed, listed = oracle_run(name)
    gt, mine = loaded_table(vh, c, pre, tmp_path)
    before = gt.counters()
    gt.delete_blocks(dev(torch_cuda, c.key_list()))
    same_as_oracle(c, gt, mine, post, c.facts["doomed"], freed, before)
    index_and_way_back(c, gt, listed, c.facts["back"], pre)
    if c.family == "P":
        assert len({(n, m) for _, n, m in c.facts["plan"]}) == 62
    if c.family == "C":
        assert len(c.facts["masks"]) == len(set(c.facts["masks"])) == len(c.facts["homes"])
    if c.family == "I":
        assert len(set(c.facts["combos"])) == 64
    print(f"{c.name}: {len(c.insert)} entries, {len(c.keys)} keys listed, {freed} freed; table, voxels, index and way back compared")
    gt.close()


def test_all_subsets_are_covered():
    assert sorted(m for p in range(2) for m in case(f"C-{p}").facts["masks"]) == MASKS == case("C-bucket4").facts["masks"]
    assert len({x for p in range(8) for x in case(f"I-{p}").facts["combos"]}) == 512


# ---- 2. the wrapped chain, on a table and on a shard -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shard", [False, True], ids=["table", "shard"])
def test_delete_blocks_on_the_wrapped_chain(vh, torch_cuda, tmp_path, shard):
    """Every one of the 128 subsets of the chain on the last bucket (of the table; of a vh_create_shard context whose range
    starts above 0, with keys of the other shard in the list), a reload each."""
    done = 0
    for mask in MASKS:
        c, pre, post, freed, listed = oracle_run(f"W-{'shard' if shard else 'table'}-{mask}")
        gt, mine = loaded_table(vh, c, pre, tmp_path)
        assert (gt.bucket_range[0] > 0) == shard
        before = gt.counters()
        gt.delete_blocks(dev(torch_cuda, c.key_list()))
        same_as_oracle(c, gt, mine, post, c.facts["doomed"], freed, before)
        index_and_way_back(c, gt, listed, c.facts["back"], pre)
        gt.close()
        done += 1
    assert done == 128
    print(f"wrapped chain on a {'shard' if shard else 'table'}: {done} subsets compared")


# ---- 3. a colour volume --------------------------------------------------------------------------------------------------------------------
def test_delete_blocks_with_a_colour_volume(vh, torch_cuda):
    """The plain buckets again, streamed in with colour words (the placement is the GPU's own, so the expectation is
    expected_plain on the downloaded pre-state): freed blocks' words become 0, the survivors' stay, although their entries move."""
    c = case("P-shuffled")
    gt = vh.SDFHashtable(c.params(vh), c.W, c.H, c.sem)
    vox = np.zeros((len(c.insert), 512), mm.VOXEL)
    for i, k in enumerate(c.insert):
        vox["sdf"][i], vox["weight"][i] = GC.pattern_block(k, i)
    colors = (np.arange(len(c.insert) * 512, dtype=U).reshape(-1, 512) * U(2654435761)) | U(1 << 24)      # count >= 1: no word is 0
    st = gt.stream_in({"keys": np.array(c.insert, np.int32), "voxels": vox, "colors": colors})
    assert st["placed"] == len(c.insert) and gt.has_color()
    pre, col0 = snapshot(gt), gt.color_volume().reshape(-1, 512)
    before = gt.counters()
    gt.delete_blocks(dev(torch_cuda, c.key_list()))
    post, col1 = snapshot(gt), gt.color_volume().reshape(-1, 512)
    k = gt.counters()
    doomed = c.facts["doomed"]
    assert GC.check_after(pre, post, doomed, c.shape, (k["last_freed"], before["freed_total"], k["freed_total"])) == len(doomed)
    assert np.array_equal(post["table"], GC.expected_plain(pre["table"], doomed, 5))
    used0, used1 = pre["table"][pre["table"]["ptr"] != -1], post["table"][post["table"]["ptr"] != -1]
    by_key = {tuple(k): i for i, k in enumerate(c.insert)}
    for e in used1:
        assert np.array_equal(col1[e["ptr"] // 512], colors[by_key[tuple(e["pos"].tolist())]])
    gone = [int(e["ptr"]) // 512 for e in used0 if tuple(e["pos"].tolist()) in doomed]
    assert len(gone) == len(doomed) and col0[gone].all() and not col1[gone].any()
    moved = sum(1 for i in np.nonzero(post["table"]["ptr"] != -1)[0] if post["table"]["ptr"][i] != pre["table"]["ptr"][i])
    assert moved > 50
    gt.close()


# ---- 4. garbage_collect: voxels that decide, behind every producer of the compact list ----------------------------------------------
PRODUCERS = ["step-level"] + list(FORMS) + ["pipelined-pending"]


def produce_list(torch, gt, c, producer):
    """The compact list of the case's pose, by the step-level flatten or by a whole frame with an all-invalid vertex map."""
    blank = dev(torch, np.zeros((c.H, c.W, 4), np.float32))
    if producer == "step-level":
        gt.set_pose(c.pose)
        assert gt.flatten() == len(c.insert)
    elif producer == "pipelined-pending":
        # Left pending: a batch flushes at its end only where the option "pipeline" was 0 before it (producer_options sets it
        # to 1), and the launch is pipelined where the frame is fused, the walk is 3 or 4 and the image's few claim tiles fit
        # one launch -- the kernel time below shows that it was.  Nothing between here and the collection reads a counter or
        # synchronises (either would settle the frame first), so vh_garbage_collect's own settle() is what completes it.
        gt.set_profiling(True)
        gt.integrate_batch([c.pose], [blank])
    else:
        gt.integrate(c.pose, blank)
        assert gt.counters()["occupied"] == len(c.insert)
    return blank


def producer_options(producer):
    if producer == "step-level":
        return {}
    if producer == "pipelined-pending":
        return dict(fused_frame=1, flatten_variant=4, pipeline=1)
    return dict(fused_frame=FORMS[producer][0], flatten_variant=FORMS[producer][1])


@pytest.mark.parametrize("threshold", list(GC.THRESHOLDS))
@pytest.mark.parametrize("producer", PRODUCERS)
def test_garbage_collect(vh, torch_cuda, tmp_path, producer, threshold):
    c, pre, post, freed, listed = oracle_run("V", threshold)
    gt, mine = loaded_table(vh, c, pre, tmp_path, **producer_options(producer))
    before = gt.counters()
    keep = produce_list(torch_cuda, gt, c, producer)
    gt.garbage_collect(c.threshold)
    same_as_oracle(c, gt, mine, post, c.facts["doomed"], freed, before)
    decided = GC.deciding_voxels(c)
    assert len(decided) == 2 * 512
    if producer == "pipelined-pending":
        kt = gt.kernel_times()
        assert kt["frame_pipelined_ms"] > 0 and kt["frame_commit_integrate_ms"] == 0 and kt["frame_scan_claim_ms"] == 0, kt
    if c.facts["doomed"] != set(c.insert) or producer == "step-level":     # (an emptied table: the index check once is enough)
        index_and_way_back(c, gt, listed, [sorted(c.facts["doomed"])], pre)
    print(f"{c.name} behind {producer}: {len(c.insert)} blocks listed, {freed} freed, {len(decided)} decided by one voxel")
    del keep
    gt.close()


@pytest.mark.parametrize("producer", ["step-level", "fused-indexed-walk"])
def test_garbage_collect_more_blocks_than_workgroups(vh, torch_cuda, tmp_path, producer):
    """More listed blocks than gc_identify_kernel's 2048 workgroups, the last 300 of the list decided by single voxels."""
    c, pre, post, freed, listed = oracle_run("V", "T", big=True)
    assert len(c.insert) >= 2049
    gt, mine = loaded_table(vh, c, pre, tmp_path, **producer_options(producer))
    before = gt.counters()
    keep = produce_list(torch_cuda, gt, c, producer)
    gt.garbage_collect(c.threshold)
    same_as_oracle(c, gt, mine, post, c.facts["doomed"], freed, before)
    del keep
    gt.close()


# ---- 5. the grid: more listed buckets than the sweep's 65 536 lanes -------------------------------------------------------------------
G_BUCKETS, G_POOL = 1 << 18, 133000
G_PLAN = (("one doomed", 150, 1), ("both doomed", 100, 2), ("slot 0 doomed", 65700, 2), ("slot 1 doomed", 100, 2),
          ("both stay", 300, 2), ("one stays", 400, 1))
G_LISTED, G_MOVERS, G_DOOMED, G_KEYS = 150 + 100 + 65700 + 100, 65700, 150 + 200 + 65700 + 100, 150 + 200 + 131400 + 200 + 600 + 400


def test_more_listed_buckets_than_lanes(vh, torch_cuda):
    """2^18 buckets x 2 without the list, 132 950 blocks made on the device, 66 150 keys deleted in one call: 66 050 listed
    buckets, so the sweep's lanes stride and 514 listed indices lie beyond 65 536.  The order of the sweep list is the
    atomics' and cannot be read back, so the plan makes the claim hold in every order: only 350 of the listed buckets move
    nothing, the other 65 700 move their survivor from slot 1 to slot 0 -- at least 514 - 350 = 164 of those were served at
    a listed index beyond 65 536.  (That takes two blocks for nearly every listed bucket: a pool of 133 000, not the 70 000 a
    plan of mostly single-key buckets would need, which guarantees no mover beyond the stride.)  Against expected_plain on
    the downloaded pre-state, and the state check."""
    torch = torch_cuda
    t0 = time.perf_counter()
    kinds, first = [], 0
    for kind, (_, buckets, per) in enumerate(G_PLAN):
        kinds.append((first, first + buckets, per))
        first += buckets
    idx = np.arange(first)
    bucket = 3 * idx + 1                                                    # spread over the table, distinct
    per = np.concatenate([np.full(hi - lo, p) for lo, hi, p in kinds])
    b2 = np.concatenate([bucket, bucket[per == 2]])
    x = np.concatenate([np.full(len(bucket), 1), np.full(int((per == 2).sum()), 2)]).astype(np.int64)
    m = G_BUCKETS - 1
    z = ((b2 ^ (x * 73856093)) & m) * pow(83492791, -1, G_BUCKETS) & m      # mesh_models.key_for_bucket, vectorised (y = 0)
    keys = np.stack([x, np.zeros_like(x), z], 1).astype(np.int32)
    assert np.array_equal(mm.hash_block(keys, G_BUCKETS), b2) and len(keys) == G_KEYS <= G_POOL
    n = len(keys)
    words = torch.zeros((n, mm.RECORD_BYTES // 4), dtype=torch.int32, device="cuda")
    words[:, :3] = torch.from_numpy(keys).cuda()
    words[:, 4:] = (torch.arange(n, device="cuda", dtype=torch.int32)[:, None] * 1024
                    + torch.arange(1024, device="cuda", dtype=torch.int32)[None, :] + 1)      # no zero word, every block its own
    gt = vh.SDFHashtable(vh.default_params(numBuckets=G_BUCKETS, bucketSize=2, numVoxelBlocks=G_POOL), 64, 48, 1)
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st = gt.stream_in_from(words.view(torch.uint8).reshape(n, mm.RECORD_BYTES), n, status=status)
    assert st["placed"] == n and bool((status == PLACED).all())
    del words
    pre = snapshot(gt)
    rows = pre["table"].reshape(-1, 2)
    doomed = []
    for (lo, hi, p), (what, _, _) in zip(kinds, G_PLAN):
        r = rows[bucket[lo:hi]]
        assert ((r["ptr"] != -1).sum(1) == p).all(), what
        if what in ("one doomed", "slot 0 doomed"):
            doomed.append(r["pos"][:, 0])
        elif what == "both doomed":
            doomed += [r["pos"][:, 0], r["pos"][:, 1]]
        elif what == "slot 1 doomed":
            doomed.append(r["pos"][:, 1])
    doomed = np.concatenate(doomed)
    listed = G_LISTED
    assert len(doomed) == G_DOOMED and listed > 65536
    assert listed - G_MOVERS < listed - 65536                              # fewer listed buckets that move nothing than indices beyond the stride
    k4 = np.zeros((len(doomed), 4), np.int32)
    k4[:, :3] = doomed[np.random.RandomState(3).permutation(len(doomed))]
    before = gt.counters()
    t1 = time.perf_counter()
    gt.delete_blocks(dev(torch, k4))
    gt.synchronize()
    t2 = time.perf_counter()
    post = snapshot(gt)
    k = gt.counters()
    dset = set(map(tuple, doomed.tolist()))
    want = GC.expected_plain(pre["table"], dset, 2)
    assert np.array_equal(post["table"], want)
    shape = dict(numBuckets=G_BUCKETS, bucketSize=2, listSize=0, overflow=False, lo=0, hi=G_BUCKETS)
    assert GC.check_after(pre, post, dset, shape, (k["last_freed"], before["freed_total"], k["freed_total"])) == G_DOOMED
    lo, hi, _ = kinds[2]
    after = post["table"].reshape(-1, 2)[bucket[lo:hi]]
    movers = int((after["ptr"][:, 0] == rows[bucket[lo:hi]]["ptr"][:, 1]).sum())
    assert movers == G_MOVERS and movers - 65536 >= 164                    # so at least 164 movers were served beyond listed index 65 536
    lo, hi, _ = kinds[4]
    assert (post["table"].reshape(-1, 2)[bucket[lo:hi]]["ptr"] != -1).all()  # survivors in both slots
    print(f"grid: {listed} listed buckets, {len(doomed)} keys, {movers} survivors moved from slot 1 to slot 0; "
          f"delete_blocks {1e3 * (t2 - t1):.1f} ms, whole test {time.perf_counter() - t0:.1f} s")
    gt.close()
