"""The shadow model of tests/test_gpu_lifecycle.py: one model on the CPU that is carried through the same calls as the GPU context
and is advanced ONLY from its own state, by the rules the repository already has in executable form -- the oracle (frames,
deletion, insertion), deintegrate_ref, color_ref, merge_ref, merge_color_ref, stream_ref.  Nothing here reads a GPU result.

Shadow holds an OracleTable (the hash table, the heap and the TSDF volume), a colour volume indexed by the oracle's ptr, the
has_color flag, and the compact list as keys (the oracle's own list is the last flatten's; vh_merge and the de-integrations leave
lists the oracle has no call for, so the list lives here and vh_garbage_collect's rule is applied to it).

table_invariants() checks a downloaded GPU state (merge_color_cases.snapshot) for the structure every call must leave."""
import numpy as np

import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as D
import merge_color_cases as CC
import merge_color_ref as M
import merge_ref as R
import mesh_models as MM
import stream_ref as S

F = np.float32
U = np.uint32
W, H = DC.W, DC.H
SENTINEL = 0x7FFFFFFF

# variant -> (table parameters, overflow list)
VARIANTS = {"A": (dict(DC.KW, numVoxelBlocks=2048), False),
            "B": (dict(numBuckets=257, bucketSize=4, numVoxelBlocks=4096), True)}


def keys_of(entries):
    return [tuple(k) for k in np.asarray(entries["pos"]).reshape(-1, 3).tolist()]


class Shadow:
    def __init__(self, oracle, variant, sem, kw=None):
        base, self.overflow = VARIANTS[variant]
        kw = base if kw is None else kw
        self.oracle, self.variant, self.sem = oracle, variant, sem
        self.ot = oracle.OracleTable(oracle.default_params(**kw), W, H, sem)
        self.ot.set_projection(DC.projection(sem))
        self.ot.set_overflow(self.overflow)
        self.params = self.ot.params
        self.vs = F(self.params.voxelSize)
        self.proj = DC.projection(sem)
        self.color = np.zeros(self.params.numVoxelBlocks * 512, U)
        self.has_color = False
        self.compact = []                       # keys of the compact list
        self.inserted = False                   # a call has placed blocks whose slot the rule leaves free
        self.refused = 0                        # keys insert_blocks did not place
        # block reuse: ids freed by a removal, those of them handed out again while has_color, and whether colour went in
        self.freed_ids, self.reused_ids, self.reuse_coloured = set(), set(), False

    def close(self):
        self.ot.close()

    # ---- the state --------------------------------------------------------------------------------------------------------------
    def table(self):
        return self.ot.hash_table()

    def live(self):
        t = self.table()
        return t[t["ptr"] != -1]

    def live_keys(self):
        return self.live()["pos"].copy()

    def ptr_of(self):
        return {k: int(p) for k, p in zip(keys_of(self.live()), self.live()["ptr"].tolist())}

    def model(self):
        return CC.model_of(self.table(), self.ot.sdf_blocks(), self.color)

    def occupied(self):
        return len(self.compact)

    def _ids(self):
        return set((self.live()["ptr"] // 512).tolist())

    def _handed_out(self, before):
        """Book-keeping after a call that may have taken blocks off the heap."""
        new = self._ids() - before
        if self.has_color:
            self.reused_ids |= new & self.freed_ids
        self.freed_ids -= new

    def _visible(self, pose):
        inv = self.oracle.invert4x4(pose)
        tab = self.table()
        return tab[D.visible_entries(tab, self.params, self.sem, self.proj, pose, inv, W, H)].copy(), inv

    def _flatten(self, pose):
        """vh_set_pose + vh_flatten: the visible entries, in table order, which become the compact list."""
        entries, inv = self._visible(pose)
        self.compact = keys_of(entries)
        return entries, inv

    # what a call would change, without changing it (the plans draw only steps that do something)
    def would_deintegrate(self, pose, depth_source):
        entries, inv = self._visible(pose)
        _, stats = D.apply_frame(self.ot.sdf_blocks(), entries, self.params, self.sem, self.proj, inv, pose, depth_source, 0, -1)
        return stats["reset"] + stats["partial"]

    def would_color(self, pose, depth_source, rgba, band, weight_max):
        entries, inv = self._visible(pose)
        new, _ = CR.integrate(self.color, self.ot.sdf_blocks(), entries, self.params, self.sem, self.proj, inv, depth_source, rgba, band,
                              weight_max)
        return int((new != self.color).sum())

    def would_decolor(self, pose, depth_source, rgba, band):
        entries, inv = self._visible(pose)
        new, _ = M.deintegrate(self.color, self.ot.sdf_blocks(), entries, self.params, self.sem, self.proj, inv, depth_source, rgba, band)
        return int((new != self.color).sum())

    def _colour_written(self, old):
        changed = np.nonzero(self.color != old)[0]
        if len(changed) and self.reused_ids & set((changed // 512).tolist()):
            self.reuse_coloured = True
        return len(changed)

    # ---- frames ------------------------------------------------------------------------------------------------------------------
    def set_alloc_band(self, band):
        self.ot.set_alloc_band(band)

    def integrate(self, pose, verts):
        before = self._ids()
        self.ot.integrate(pose, verts)
        self.compact = keys_of(self.ot.compact())
        self._handed_out(before)

    def integrate_batch(self, frames):
        for pose, verts in frames:
            self.integrate(pose, verts)

    # ---- taking a frame back out -------------------------------------------------------------------------------------------------
    def deintegrate(self, pose, depth_source):
        """depth_source: the .z plane of a vertex map (vh_deintegrate) or (d16, k_inv) (vh_deintegrate_depth).  Returns the
        number of voxels that changed."""
        entries, inv = self._flatten(pose)
        vox, stats = D.apply_frame(self.ot.sdf_blocks(), entries, self.params, self.sem, self.proj, inv, pose, depth_source, 0, -1)
        self.ot.sdf_blocks()[:] = vox
        self.last_voxels = stats["reset"] + stats["partial"]          # (for the compositions, which return their colour count)
        return self.last_voxels

    # ---- colour ------------------------------------------------------------------------------------------------------------------
    def integrate_color(self, pose, depth_source, rgba, band, weight_max):
        entries, inv = self._flatten(pose)
        old = self.color
        self.color, _ = CR.integrate(old, self.ot.sdf_blocks(), entries, self.params, self.sem, self.proj, inv, depth_source, rgba,
                                     band, weight_max)
        self.has_color = True
        return self._colour_written(old)

    def deintegrate_color(self, pose, depth_source, rgba, band):
        assert self.has_color
        entries, inv = self._flatten(pose)
        old = self.color
        self.color, _ = M.deintegrate(old, self.ot.sdf_blocks(), entries, self.params, self.sem, self.proj, inv, depth_source, rgba, band)
        return self._colour_written(old)

    def clear_color(self):
        self.color[:] = 0

    # ---- the compositions, in the order the header defines them -----------------------------------------------------------------
    def integrate_depth_color(self, pose, d16, verts, rgba, band, weight_max):
        self.integrate(pose, verts)
        return self.integrate_color(pose, (d16, DC.k_inv()), rgba, band, weight_max)

    def deintegrate_depth_color(self, pose, d16, rgba, band):
        n = self.deintegrate_color(pose, (d16, DC.k_inv()), rgba, band)
        self.deintegrate(pose, (d16, DC.k_inv()))
        return n + self.integrate_color(pose, (d16, DC.k_inv()), rgba, band, 0)

    def reintegrate_depth(self, old_pose, new_pose, d16, verts):
        n = self.deintegrate(old_pose, (d16, DC.k_inv()))
        self.integrate(new_pose, verts)
        return n

    def reintegrate_depth_color(self, old_pose, new_pose, d16, verts, rgba, band, weight_max):
        n = self.deintegrate_depth_color(old_pose, d16, rgba, band)
        return n + self.integrate_depth_color(new_pose, d16, verts, rgba, band, weight_max)

    # ---- removal -----------------------------------------------------------------------------------------------------------------
    def delete_blocks(self, keys):
        """The oracle's deletion; the colour of the freed blocks goes with them.  Returns the number freed."""
        ptr = self.ptr_of()
        gone = [ptr[tuple(k)] for k in keys if tuple(k) in ptr]
        freed = self.ot.delete_blocks([tuple(k) for k in keys])
        assert freed == len(gone)
        for p in gone:
            self.color[p:p + 512] = 0
            self.freed_ids.add(p // 512)
        self.compact = []
        return freed

    def collectable(self, threshold):
        """vh_garbage_collect's rule over the compact list: no weight anywhere, or min |sdf| over the weighted voxels >= threshold."""
        ptr, vox = self.ptr_of(), self.ot.sdf_blocks()
        out = []
        for k in self.compact:
            v = vox[ptr[k]:ptr[k] + 512]
            held = v["weight"] > F(0.0)
            if not held.any() or np.abs(v["sdf"][held]).min() >= F(threshold):
                out.append(k)
        return out

    def garbage_collect(self, threshold):
        return self.delete_blocks(self.collectable(threshold))

    # ---- streaming ---------------------------------------------------------------------------------------------------------------
    def stream_count(self, region):
        return len(S.selection_of_table(self.table(), region, self.vs))

    def stream_out(self, region, capacity=None):
        """(chunk as SDFHashtable.stream_out returns it, in the oracle's table order).  The colour travels if there is any."""
        tab = self.table()
        order = S.selection_of_table(tab, region, self.vs)
        taken = order if capacity is None else order[:capacity]
        keys = keys_of(tab[taken])
        chunk = S.chunk_of(self.model(), keys, self.has_color)
        chunk["selected"] = len(order)
        self.delete_blocks(keys)
        return chunk

    def stream_in(self, chunk):
        """The statuses by the rule, the PLACED records inserted and filled.  Returns (status [n], placed)."""
        status, _ = S.stream_in(self.model(), chunk)
        keys = keys_of({"pos": chunk["keys"]})
        placed = [i for i, s in enumerate(status.tolist()) if s == S.PLACED]
        before = self._ids()
        got = self.ot.insert_blocks([keys[i] for i in placed])
        self.refused += len(placed) - got
        if chunk.get("colors") is not None:
            self.has_color = True
        self._handed_out(before)
        ptr, vox = self.ptr_of(), self.ot.sdf_blocks()
        for i in placed:
            if keys[i] not in ptr:
                continue                                                    # (refused: the CPU test fails on `refused`)
            p = ptr[keys[i]]
            vox[p:p + 512] = chunk["voxels"][i]
            if chunk.get("colors") is not None:
                self.color[p:p + 512] = chunk["colors"][i]
        self.compact = []
        self.inserted |= bool(placed)
        return status, len(placed)

    # ---- one model into another --------------------------------------------------------------------------------------------------
    def merge(self, src_model, src_vs, T, mode, colors, weight_max=255):
        """vh_merge / vh_merge_color of the fixed coloured src.  Returns stats: candidates (records), allocated, blocks, updated
        (blocks the model held before that received the update)."""
        cand, records = R.candidates(src_model.keys(), T, F(src_vs), self.vs)
        held = set(keys_of(self.live()))
        before = self._ids()
        missing = sorted(cand - held)
        got = self.ot.insert_blocks(missing)
        self.refused += len(missing) - got
        if colors and src_model:
            self.has_color = True                                           # the volume appears with the first coloured merge
        self._handed_out(before)
        model = self.model()
        present = sorted(cand & model.keys())
        Tinv = self.oracle.invert4x4(T)
        args = (present, Tinv, F(src_vs), self.vs, self.params.truncation, self.params.integrationWeightMax, mode)
        if colors:
            out, _, _ = M.apply(model, src_model, *args, weight_max)
        else:
            geo, _ = R.apply(M.geometry(model), M.geometry(src_model), *args)
            out = {k: (geo[k][0], geo[k][1], model[k][2]) for k in model}
        ptr, vox = self.ptr_of(), self.ot.sdf_blocks()
        old = self.color.copy()
        for k in present:
            p = ptr[k]
            vox["sdf"][p:p + 512], vox["weight"][p:p + 512] = out[k][0], out[k][1]
            self.color[p:p + 512] = out[k][2]
        if colors:
            self._colour_written(old)
        self.compact = present
        self.inserted |= got > 0
        return dict(candidates=records, allocated=got, blocks=len(present), updated=len(set(present) & held))

    # ---- saved models ------------------------------------------------------------------------------------------------------------
    def reload(self, with_color):
        """save_snapshot (+ save_color) and load_snapshot (+ load_color): the model is what it was, the compact list is empty; a
        snapshot loaded without its colour file has no colour."""
        self.ot.delete_blocks([])
        self.compact = []
        if not with_color:
            self.color[:] = 0


# ---- the structure of a downloaded state ---------------------------------------------------------------------------------------
def table_invariants(snap, params, overflow, bucket_lo=0):
    """Raises AssertionError naming the clause a downloaded state (merge_color_cases.snapshot, or the same keys from the oracle)
    breaks."""
    tab, heap, c = snap["table"], np.asarray(snap["heap"]).astype(np.int64), snap["counters"]
    bs, nb, pool, L = int(params.bucketSize), int(params.numBuckets), int(params.numVoxelBlocks), int(params.attachedLinkedListSize)
    n = len(tab)
    live = np.nonzero(tab["ptr"] != -1)[0]
    keys = keys_of(tab[live])
    assert len(set(keys)) == len(keys), "a key appears twice"
    home = np.asarray(MM.hash_block(tab["pos"][live].astype(np.int64), nb)).astype(np.int64) - bucket_lo if len(live) else np.zeros(0, np.int64)
    away = live[(live // bs) != home]
    if len(away):
        assert overflow, "an entry outside its home bucket without the overflow list"
    chained = set()
    for h in sorted(set((np.nonzero(tab["offset"] != 0)[0] // bs).tolist()) | set(home[(live // bs) != home].tolist())):
        last = h * bs + bs - 1
        i = last
        for _ in range(L):
            off = int(tab["offset"][i])
            if off == 0:
                break
            i = (last + off) % n
            assert tab["ptr"][i] != -1, "a chain links to a free slot"
            assert int(MM.hash_block(tab["pos"][i:i + 1].astype(np.int64), nb)[0]) - bucket_lo == h, "a chained entry of another bucket"
            chained.add(i)
    assert set(away.tolist()) <= chained, "an entry neither in its home bucket nor on its chain"
    if overflow:
        heads = np.nonzero(tab["offset"] != 0)[0]
        assert (tab["ptr"][heads] != -1).all(), "a free slot carries a link"
    else:
        used = (tab["ptr"] != -1).reshape(-1, bs)
        assert not (used[:, 1:] & ~used[:, :-1]).any(), "a hole before an entry in a bucket"
    free = tab[tab["ptr"] == -1]
    assert (free["pos"] == SENTINEL).all() and (free["offset"] == 0).all(), "a free entry without the sentinel"
    ptr = tab["ptr"][live].astype(np.int64)
    assert (ptr % 512 == 0).all() and len(set(ptr.tolist())) == len(ptr), "ptrs are not distinct multiples of 512"
    hc = int(c["heap_counter"])
    on_heap, held = heap[:hc + 1], ptr // 512
    both = set(on_heap.tolist()) & set(held.tolist())
    assert not both, f"a block both free and referenced: {sorted(both)[:4]}"
    assert len(set(on_heap.tolist())) == len(on_heap), "a block twice on the heap"
    missing = set(range(pool)) - set(on_heap.tolist()) - set(held.tolist())
    assert not missing, f"a block neither on the heap nor referenced: {sorted(missing)[:4]}"
    assert set(on_heap.tolist()) | set(held.tolist()) == set(range(pool)), "a block id outside the pool"
    assert pool - 1 - hc == len(live), "heap_counter does not match the allocated entries"
    if "allocated_total" in c:
        assert c["allocated_total"] - c["freed_total"] == len(live), "allocated_total - freed_total is not the allocated entries"
        for name in ("heap_exhausted", "bin_overflow", "cand_overflow", "spin_timeouts"):
            assert c[name] == 0, name
    compact = snap.get("compact")
    if compact is not None and len(compact):
        ck = keys_of(compact)
        assert len(set(ck)) == len(ck), "the compact list holds a duplicate"
        assert set(ck) <= set(keys), "the compact list holds an entry that is not allocated"
        at = dict(zip(keys, ptr.tolist()))
        assert all(at[k] == int(p) for k, p in zip(ck, compact["ptr"].tolist())), "a compact entry with a stale ptr"


def oracle_snapshot(shadow):
    """The shadow's oracle in the form table_invariants takes."""
    ot = shadow.ot
    return dict(table=ot.hash_table().copy(), heap=ot.heap().copy(), counters=dict(heap_counter=ot.heap_counter()), compact=None)
