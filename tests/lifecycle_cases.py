"""The plans of tests/test_lifecycle_ref_cpu.py and tests/test_gpu_lifecycle.py: one sequence of about 40 calls per (variant,
semantics, seed), drawn from numpy.random.RandomState and from the SHADOW's state only (tests/lifecycle_ref.py), so that the CPU
test and the GPU test run the same steps.  A Sequence draws a step, advances its shadow by it, writes what the shadow expects of
the call into step["expect"] and yields the step; a reader step leaves the shadow alone.

A sequence is a prelude (a fused, coloured model), then a shuffled queue of single steps -- every kind of KINDS comes up in four
of the six seeds -- and of motifs, short runs of adjacent steps that the tests need next to each other (PAIRS).  A step that
would do nothing now (a removal that frees nothing, a de-integration of a frame the model no longer holds, ...) is put back and
tried again later.  Variant B (crowded buckets, chains) draws no frame after the first call that inserted blocks: under chains a
frame's winners may depend on the layout, which the rule leaves free.

A worked example, B / semantics 1 / seed 1.  After the prelude (three batches of three frames, one RGB-D frame) items() gives
    integrate_depth_color, deintegrate_color, extract_mesh, integrate, deintegrate_depth_color, steps, pipeline, integrate_batch,
    deintegrate, fused_frame, set_alloc_band, raycast, delete_blocks | stream_out+piped+fused+frame!+stream_in | mesh_count,
    walk_reverse, extract_mesh_indexed, integrate_color_map, stream_out+stream_out+stream_in+stream_in, clear_color,
    garbage_collect, stream_out, cast_rays, stream_in, reload, sample_sdf
rank() made the three parts: first whatever claims blocks as a frame does or needs a fused frame (with a random half of the
neutral items), then the one motif that goes from a frame to an insertion, then the items that insert (with the other half).
steps() walks this list.  Before an item, enable() may add a helper: an RGB-D frame if `deintegrate_color` finds no coloured frame
left, a stream_out if `stream_in` has no chunk stored, in B a stream_out of the half of the model far from src if no transform
gives a merge room (the "again" it returns asks for one more cut while more than 300 blocks are left).  Then the item's first
step is drawn; if it has nothing to do now (`garbage_collect` with nothing collectable, say) the item goes to the back of the
queue, and once a whole round was put back the rest is recorded in `dropped`.  A motif whose later step cannot be drawn is
broken off there and recorded too; tests/test_lifecycle_ref_cpu.py asserts that every pair still occurs."""
import numpy as np

import deintegrate_cases as DC
import lifecycle_ref as LR
import merge_cases as MC
import merge_color_cases as CC
import merge_ref as R
import stream_ref as S
from voxelhashing_demo_amd import synth

F = np.float32
U = np.uint32
W, H = DC.W, DC.H
SEEDS = [0, 1, 2, 3, 4, 5]
REDRAWN = {("A", 0, 2): 1}                   # sequences drawn again because a condition of tests/test_lifecycle_ref_cpu.py failed (a frame filled a bucket of A)
SALT = 0                                     # moves every sequence's draws: chosen so that tests/test_lifecycle_ref_cpu.py's conditions hold

FRAMES = ["integrate_depth", "integrate", "integrate_batch", "steps"]
DEINT = ["deintegrate", "deintegrate_depth"]
COLOUR = ["integrate_color", "integrate_color_map", "deintegrate_color"]
COMPOSED = ["integrate_depth_color", "deintegrate_depth_color", "reintegrate_depth", "reintegrate_depth_color"]
REMOVALS = ["delete_blocks", "garbage_collect", "stream_out"]
INSERTS = ["stream_in", "merge", "merge_color"]
OTHER = ["reload", "clear_color"]
OPTIONS = ["pipeline", "fused_frame", "flatten_variant", "walk_nt", "walk_reverse", "set_alloc_band"]
READERS = ["raycast", "sample_sdf", "sample_color", "sample_lattice", "cast_rays", "mesh_count", "extract_mesh", "extract_mesh_indexed",
           "esdf_lattice", "stream_count"]
KINDS = FRAMES + DEINT + COLOUR + COMPOSED + REMOVALS + INSERTS + OTHER + OPTIONS + READERS
ALLOCATING = set(FRAMES) | {"integrate_depth_color", "reintegrate_depth", "reintegrate_depth_color"}      # calls that claim blocks as frames do
CHANGING = set(KINDS) - set(OPTIONS) - set(READERS)

PENDING_BEFORE = ["deintegrate", "deintegrate_color", "merge", "stream_out", "stream_in", "esdf_lattice", "sample_sdf", "extract_mesh",
                  "cast_rays"]
# motifs: runs of adjacent steps; "frame!" is a plain frame left pending, "frame" one that is compared; "piped" / "fused" set the
# option to 1.  A plain frame stays in flight only with "pipeline" AND "fused_frame" on and flatten_variant 3 or 4 (the only values
# the plans set), in a table the one-launch frame takes: bucketSize <= 16 and, with the overflow list, at most 512 claim + walk
# workgroups -- 12 image tiles + 1 or 2 walk workgroups here (pipeline_applies / can_pipeline in vh_api_frame.hip)
MOTIFS = ([["stream_out", "stream_in", "garbage_collect"],
           ["stream_out", "stream_out", "stream_in", "stream_in"],
           ["merge", "stream_out"],
           ["stream_out", "extract_mesh", "stream_out"],
           ["stream_out", "deintegrate_depth", "garbage_collect", "stream_in"],
           ["deintegrate", "garbage_collect"],
           ["reload", "integrate_color"],
           ["fused", "stream_out", "stream_in", "frame"],
           ["fused", "merge", "frame"]]
          + [(["stream_out"] if x == "stream_in" else []) + ["piped", "fused", "frame!", x] for x in PENDING_BEFORE])
A_ONLY = (7, 8)
NEED_FUSED = set(DEINT) | {"reintegrate_depth", "deintegrate_depth_color", "reintegrate_depth_color"}
NEED_COLOUR = {"deintegrate_color", "deintegrate_depth_color", "reintegrate_depth_color", "clear_color"}


def frames_of(oracle, variant):
    """[(pose, d16, verts)]: the three frames of deintegrate_cases for A, three room frames of test_gpu_sequences' loop for B."""
    if variant == "A":
        return DC.frames(oracle)
    key = ("B", W, H)
    if key not in DC._FRAMES:
        out = []
        for pose in synth.camera_loop(40)[::4][:3]:
            d16 = DC.sensor_image(pose)
            out.append((pose, d16, oracle.preprocess(d16, DC.k_inv())[0]))
        DC._FRAMES[key] = out
    return DC._FRAMES[key]


_SRC = {}


def source_model(oracle, variant, sem):
    """The fixed coloured src of the merges: frame 0 fused and coloured once in a roomy table with the variant's voxel size (the
    oracle's TSDF, color_ref's colour); for B the 12 blocks nearest the middle, so that the crowded table has room for what a
    merge allocates.  {key: (sdf, weight, colour)}; the GPU test hands it to a src context through stream_in."""
    if (variant, sem) not in _SRC:
        vs = LR.VARIANTS[variant][0].get("voxelSize", oracle.default_params().voxelSize)
        sh = LR.Shadow(oracle, "A", sem, kw=dict(DC.KW, numVoxelBlocks=2048, voxelSize=vs))
        pose, d16, verts = frames_of(oracle, variant)[0]
        sh.integrate(pose, verts)
        sh.integrate_color(pose, (d16, DC.k_inv()), CC.image(0), 1.5 * float(sh.vs), 255)
        model = sh.model()
        sh.close()
        if variant == "B":
            keys = np.array(sorted(model), np.float64)
            near = np.argsort(np.linalg.norm(keys - keys.mean(0), axis=1), kind="stable")[:12]
            model = {tuple(int(c) for c in keys[i]): model[tuple(int(c) for c in keys[i])] for i in sorted(near.tolist())}
        _SRC[(variant, sem)] = model
    return _SRC[(variant, sem)]


class Sequence:
    def __init__(self, oracle, variant, sem, seed):
        self.oracle, self.variant, self.sem, self.seed = oracle, variant, sem, seed
        self.rng = np.random.RandomState(SALT + 10000 * (variant == "B") + 1000 * sem + seed + 100 * REDRAWN.get((variant, sem, seed), 0))
        self.shadow = LR.Shadow(oracle, variant, sem)
        self.frames = frames_of(oracle, variant)
        self.src = source_model(oracle, variant, sem)
        self.band = 1.5 * float(self.shadow.vs)
        self.transforms = [MC.TRANSFORMS[n] for n in sorted(MC.TRANSFORMS)] + [CC.CLOSE]
        self.store = []                          # chunks streamed out and not yet back
        self.fused = {}                          # (frame, pose index) -> times its depth is in the model
        self.coloured = {}                       # (frame, pose index, image) -> times its colour is in the model
        self.options = {"pipeline": 0, "fused_frame": 1}
        self.log = []
        self.dropped = []

    def close(self):
        self.shadow.close()

    # ---- the queue ---------------------------------------------------------------------------------------------------------------
    def items(self):
        deck = [[k] for j, k in enumerate(KINDS) if (j - self.seed) % len(SEEDS) < 4]
        motifs = [m for i, m in enumerate(MOTIFS) if i % len(SEEDS) == self.seed and not (self.variant == "B" and i in A_ONLY)]
        queue = deck + motifs
        self.rng.shuffle(queue)
        if self.variant == "B":                  # no frame after an insertion: the items that claim blocks as frames do come before the
            early = {id(item): int(self.rng.randint(2)) for item in queue}      # items that insert, the rest on either side
            def rank(item):
                claims = any(k in ALLOCATING or k.startswith("frame") or k in NEED_FUSED for k in item)
                inserts = any(k in INSERTS for k in item)
                return 1 if claims and inserts else 0 if claims else 2 if inserts else 2 * early[id(item)]
            queue.sort(key=rank)
        return queue

    def steps(self):
        if self.variant == "A":
            prelude = ["integrate_depth", "integrate_depth_color"]
        else:
            prelude = ["integrate_batch", "integrate_batch", "integrate_batch", "integrate_depth_color"]
        for kind in prelude:
            step = self.draw(kind, prelude=True)
            yield self.apply(step)
        # items are taken in order; one whose first step has nothing to do now goes to the back, and the loop ends when a whole
        # round of the queue was put back (those items are `dropped`; tests/test_lifecycle_ref_cpu.py bounds them)
        queue = self.items()
        tries = 0
        while queue and tries < len(queue) + 1:
            item = queue.pop(0)
            for _ in range(3):                   # ("again": B is still too crowded for a merge, cut it once more)
                helpers = self.enable(item)
                for step in helpers:
                    if step != "again":
                        yield self.apply(step)
                if "again" not in helpers:
                    break
            first = self.draw(self.real(item[0]), item[0])
            if first is None:
                queue.append(item)
                tries += 1
                continue
            tries = 0
            yield self.apply(first)
            for name in item[1:]:
                step = self.draw(self.real(name), name)
                if step is None:
                    self.dropped.append((tuple(item), name))
                    break
                yield self.apply(step)
        self.dropped += [(tuple(item), item[0]) for item in queue]

    def enable(self, item):
        """Steps that give the item something to do where the model has nothing for it: a frame for a de-integration, colour for
        a colour removal, a chunk for a stream-in, a list for a collection."""
        out = []
        frames_allowed = not (self.variant == "B" and self.shadow.inserted)
        for kind in item:
            if kind in NEED_FUSED | NEED_COLOUR and self.draw(kind) is None:
                helper = "integrate_depth_color" if frames_allowed else "integrate_color" if kind in ("deintegrate_color", "clear_color") else None
                step = helper and self.draw(helper)
                if step is not None:
                    out.append(step)
                break
        if item[0] == "stream_in" and not self.store:
            out.append(self.draw("stream_out"))
        crowded = "frame!" in item and len(self.shadow.live()) > 350
        if self.variant == "B" and any(k in ("merge", "merge_color") for k in item) and (crowded or self.draw("merge") is None):
            held = set(LR.keys_of(self.shadow.live()))
            near = any(c - held and c & held for c in (R.candidates(self.src.keys(), T, self.shadow.vs, self.shadow.vs)[0] for T in self.transforms))
            if near or crowded:                                          # the crowded table has no room for what a merge allocates
                out.append(self.draw("stream_out", "half"))
                if len(self.shadow.live()) > 300:
                    out.append("again")
            elif self.store:                                             # nothing of the model lies where src goes
                out.append(self.draw("stream_in"))
        return [s for s in out if s is not None]

    def real(self, name):
        return {"frame": "integrate_depth", "frame!": "integrate_depth", "fused": "fused_frame", "piped": "pipeline"}.get(name, name)

    # ---- drawing one step from the shadow's state --------------------------------------------------------------------------------
    def region(self):
        """A region through the live blocks as stream_cases.middle_sphere / middle_box cut them, at a quarter or a half."""
        keys = self.shadow.live_keys()
        kind, q = self.rng.randint(3), float(self.rng.choice([25, 50]))
        if kind == 0:
            big = 1 << 31
            return S.box((-big, -big, -big), (int(np.percentile(keys[:, 0], q)), big - 1, big - 1))
        centres = (8.0 * keys.astype(np.float64) + 3.5) * float(self.shadow.vs)
        c = centres.mean(axis=0).astype(F)
        r = F(np.percentile(np.linalg.norm(centres - c, axis=1), q if kind == 1 else 100.0 - q))
        return S.sphere(tuple(float(v) for v in c), float(r), invert=(kind == 2))

    def far_from_src(self):
        """The half of the live blocks farthest from the middle of src."""
        centres = (8.0 * self.shadow.live_keys().astype(np.float64) + 3.5) * float(self.shadow.vs)
        c = ((8.0 * np.array(sorted(self.src), np.float64) + 3.5) * float(self.shadow.vs)).mean(axis=0).astype(F)
        r = F(np.median(np.linalg.norm(centres - c, axis=1)))
        return S.sphere(tuple(float(v) for v in c), float(r), invert=True)

    def depth_source(self, f, sensor):
        return (self.frames[f][1], DC.k_inv()) if sensor else self.frames[f][2][..., 2]

    def draw(self, kind, role=None, prelude=False):
        """A step dict of `kind` that does something in the shadow's present state, or None."""
        rng, sh = self.rng, self.shadow
        nf = len(self.frames)
        live = len(sh.live())
        step = {"op": kind}
        if kind in ALLOCATING and self.variant == "B" and sh.inserted:
            return None
        if kind in ("integrate_depth", "integrate", "steps"):
            step.update(f=int(rng.randint(nf)))
            step["p"] = step["f"]
            if role == "frame!":
                step["pending"] = True
            elif role != "frame" and kind != "steps" and not prelude:
                step["pending"] = bool(rng.randint(2))
        elif kind == "integrate_batch":
            n = nf if prelude else int(rng.randint(1, 4))
            step.update(fs=list(range(nf)) if prelude else [int(rng.randint(nf)) for _ in range(n)])
        elif kind in DEINT:
            have = [k for k, n in sorted(self.fused.items()) if n > 0]
            rng.shuffle(have)
            for f, p in have:
                if sh.would_deintegrate(self.frames[p][0], self.depth_source(f, kind == "deintegrate_depth")) >= 100:
                    return dict(step, f=f, p=p)
            return None
        elif kind in ("integrate_color", "integrate_color_map", "integrate_depth_color"):
            f, img = (1, 1) if prelude else (int(rng.randint(nf)), int(rng.randint(5)))
            wmax = int(rng.choice([255, 255, 3]))
            step.update(f=f, p=f, img=img, wmax=wmax)
            if kind != "integrate_depth_color" and sh.would_color(self.frames[f][0], self.depth_source(f, kind == "integrate_color"),
                                                                  CC.image(img), self.band, wmax) < 100:
                return None
        elif kind in ("deintegrate_color", "deintegrate_depth_color", "reintegrate_depth_color"):
            if not sh.has_color:
                return None
            have = [k for k, n in sorted(self.coloured.items()) if n > 0 and (kind == "deintegrate_color" or self.fused.get(k[:2], 0) > 0)]
            rng.shuffle(have)
            for f, p, img in have:
                if kind != "deintegrate_color" and sh.would_deintegrate(self.frames[p][0], self.depth_source(f, True)) < 100:
                    continue
                if sh.would_decolor(self.frames[p][0], self.depth_source(f, True), CC.image(img), self.band) >= 100:
                    step.update(f=f, p=p, img=img)
                    if kind == "reintegrate_depth_color":
                        step.update(q=int(rng.randint(nf)), wmax=int(rng.choice([255, 3])))
                    return step
            return None
        elif kind == "reintegrate_depth":
            have = [k for k, n in sorted(self.fused.items()) if n > 0]
            rng.shuffle(have)
            for f, p in have:
                if sh.would_deintegrate(self.frames[p][0], self.depth_source(f, True)) >= 100:
                    return dict(step, f=f, p=p, q=int(rng.randint(nf)))
            return None
        elif kind == "delete_blocks":
            if live < 16:
                return None
            tab = sh.table()
            at = np.nonzero(tab["ptr"] != -1)[0]
            pick = at[rng.choice(len(at), size=7, replace=False)].tolist()
            home = np.asarray(LR.MM.hash_block(tab["pos"][at].astype(np.int64), sh.params.numBuckets))
            chained = at[(at // sh.params.bucketSize) != home]
            if len(chained):                                            # an entry out of a chain, and the head of one
                pick += chained[rng.choice(len(chained), size=min(2, len(chained)), replace=False)].tolist()
            step.update(keys=sorted(set(tuple(k) for k in tab["pos"][pick].tolist())))
        elif kind == "garbage_collect":
            if role is not None and self.log and self.log[-1] == "stream_in":
                return dict(step, threshold=5.0)                        # (the list is empty: the call must free nothing)
            for th in (5.0, 0.3, 0.03, 0.0):
                n = len(sh.collectable(th))
                if n >= 1 and live - n >= 8:
                    return dict(step, threshold=th)
            return None
        elif kind == "stream_out":
            if live < 24:
                return None
            for _ in range(4):
                region = self.region() if role != "half" else self.far_from_src()
                n = sh.stream_count(region)
                if n >= 1 and live - n >= 8:
                    cap = None
                    if self.variant == "B" and not sh.inserted and n >= 3 and rng.randint(2):
                        cap = n // 3                                    # (the order is the table's: only while the slots are known)
                    return dict(step, region=region, capacity=cap)
            return None
        elif kind == "stream_in":
            if sh.ot.heap_counter() < 64:
                return None
            held = sh.live_keys()
            extra = held[rng.choice(len(held), size=min(3, len(held)), replace=False)] if len(held) else np.zeros((0, 3), np.int32)
            model = sh.model()
            for which in rng.permutation(len(self.store)).tolist():
                chunk = self.augmented(self.store[which], extra, strip=rng.randint(3) == 0)
                status, _ = S.stream_in(model, chunk)
                if (status == S.PLACED).sum() >= 1 and self.has_room([tuple(k) for k in chunk["keys"][status == S.PLACED].tolist()]):
                    self.store.pop(which)
                    return dict(step, chunk=chunk)
            for _ in range(5):                                          # nothing stored can go in: blocks from elsewhere, far from every view
                keys = (rng.randint(-2000, 2000, (40, 3)) + (9000, 0, 0)).astype(np.int32)
                keys = np.array([k for k in keys.tolist() if self.has_room([tuple(k)])][:6], np.int32).reshape(-1, 3)
                if len(keys) < 6:
                    continue
                vox = np.zeros((6, 512), S.VOXEL)
                vox["sdf"], vox["weight"] = rng.standard_normal((6, 512)).astype(F), rng.randint(1, 9, (6, 512)).astype(F)
                cols = rng.randint(1, 1 << 31, (6, 512)).astype(U) if sh.has_color else None
                chunk = self.augmented({"keys": keys, "voxels": vox, "colors": cols}, extra)
                status, _ = S.stream_in(model, chunk)
                if self.has_room([tuple(k) for k in chunk["keys"][status == S.PLACED].tolist()]):
                    return dict(step, chunk=chunk)
            return None
        elif kind in ("merge", "merge_color"):
            held = set(LR.keys_of(sh.live()))
            order = list(range(len(self.transforms)))
            rng.shuffle(order)
            for t in order:
                cand, _ = R.candidates(self.src.keys(), self.transforms[t], sh.vs, sh.vs)
                if cand - held and cand & held and sh.ot.heap_counter() - len(cand - held) >= 64 and self.has_room(sorted(cand - held)):
                    return dict(step, T=self.transforms[t], mode=int(rng.randint(2)), wmax=int(rng.choice([255, 3])))
            return None
        elif kind == "reload":
            step.update(with_color=bool(sh.has_color and rng.randint(2)))
        elif kind == "clear_color":
            if not sh.has_color or not sh.color.any():
                return None
        elif kind in ("pipeline", "fused_frame"):
            step.update(value=1 if role in ("piped", "fused") else int(rng.randint(2)))
        elif kind == "flatten_variant":
            step.update(value=int(rng.choice([3, 4])))
        elif kind in ("walk_nt", "walk_reverse"):
            step.update(value=int(rng.randint(2)))
        elif kind == "set_alloc_band":
            step.update(value=float(rng.choice([0.0, 0.1])))
        elif kind in READERS:
            if live < 1:
                return None
            keys = sh.live_keys().astype(np.int64)
            vs = float(sh.vs)
            if kind == "raycast":
                step.update(f=int(rng.randint(nf)))
            elif kind in ("sample_sdf", "sample_color"):
                at = keys[rng.randint(0, len(keys), 256)]
                step.update(points=((8.0 * at + rng.uniform(-1.0, 9.0, (256, 3))) * vs).astype(F), mode=int(rng.randint(2)))
            elif kind == "sample_lattice":
                step.update(lo=(8 * keys[rng.randint(len(keys))] - 4).tolist(), dims=[16, 16, 16])
            elif kind == "cast_rays":
                from voxelhashing_demo_amd.hashtable import pinhole_rays
                K = synth.K_matrix(W, H)
                rays = pinhole_rays(self.frames[int(rng.randint(nf))][0], K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H, 0.1, 5.0)
                step.update(rays=np.ascontiguousarray(rays[rng.choice(len(rays), size=256, replace=False)]))
            elif kind in ("mesh_count", "extract_mesh", "extract_mesh_indexed"):
                lo = keys[rng.randint(len(keys))] - rng.randint(0, 2, 3)
                step.update(region=(tuple(int(v) for v in lo), tuple(int(v) + 2 for v in lo)))
            elif kind == "esdf_lattice":
                step.update(lo=(8 * keys[rng.randint(len(keys))] - 6).tolist(), dims=[20, 18, 19], radius=int(rng.randint(1, 5)))
            elif kind == "stream_count":
                step.update(region=self.region())
        return step

    def has_room(self, keys):
        """Whether the table places all of `keys` (absent ones) IN WHATEVER ORDER they are served: every key has a free slot in
        its own home bucket, the other keys of the call counted.  (Under chains a key that has to leave its home bucket takes a
        slot behind it, and whether the last keys of a crowded table still find one then depends on who was served first, which
        the rule leaves free: the GPU left a record or two UNPLACED that an insertion in key order had placed.)"""
        sh = self.shadow
        if not len(keys):
            return True
        bs = sh.params.bucketSize
        free = (sh.table()["ptr"] == -1).reshape(-1, bs).sum(1)
        need = np.bincount(np.asarray(LR.MM.hash_block(np.asarray(keys, np.int64), sh.params.numBuckets)), minlength=len(free))
        spare = 0 if sh.overflow else 1                                  # (the roomy variant never fills a bucket)
        return bool((need + spare * (need > 0) <= free).all()) and sh.ot.heap_counter() + 1 >= len(keys)

    def augmented(self, chunk, present_keys, strip=False):
        """`chunk` with its first record a second time at the end (the same contents: which of the two wins is a race) and records
        for keys the model holds, with contents of their own that must not arrive."""
        n, m = len(chunk["keys"]), len(present_keys)
        keys = np.concatenate([chunk["keys"], np.asarray(present_keys, np.int32).reshape(-1, 3), chunk["keys"][:1]])
        junk = np.zeros((m, 512), S.VOXEL)
        junk["sdf"], junk["weight"] = self.rng.standard_normal((m, 512)).astype(F), F(3.0)
        vox = np.concatenate([chunk["voxels"], junk, chunk["voxels"][:1]])
        cols = None
        if chunk["colors"] is not None and not strip:                     # (strip: the records go in without their colour)
            cols = np.concatenate([chunk["colors"], self.rng.randint(1, 1 << 31, (m, 512)).astype(U), chunk["colors"][:1]])
        return {"keys": keys, "voxels": vox, "colors": cols, "of": n}

    # ---- advancing the shadow ----------------------------------------------------------------------------------------------------
    def count(self, table, key, by):
        table[key] = table.get(key, 0) + by

    def apply(self, step):
        sh, op = self.shadow, step["op"]
        self.log.append(op + ("!" if step.get("pending") else ""))
        step["index"] = len(self.log) - 1
        ex = step["expect"] = {}
        if op in OPTIONS:
            if op == "set_alloc_band":
                sh.set_alloc_band(step["value"])
            else:
                self.options[op] = step["value"]
            step["fused"] = bool(self.options["fused_frame"])
            return step
        if op in READERS:
            return step
        before = len(sh.live())
        fr = self.frames
        f, p = step.get("f"), step.get("p")
        img = CC.image(step["img"]) if "img" in step else None
        step["fused"] = bool(self.options["fused_frame"])
        step["piped"] = bool(self.options["pipeline"])
        step["in_flight"] = bool(step.get("pending")) and step["piped"] and step["fused"]
        if op in ("integrate_depth", "integrate", "steps"):
            sh.integrate(fr[f][0], fr[f][2])
            self.count(self.fused, (f, f), 1)
        elif op == "integrate_batch":
            sh.integrate_batch([(fr[i][0], fr[i][2]) for i in step["fs"]])
            for i in step["fs"]:
                self.count(self.fused, (i, i), 1)
        elif op in DEINT:
            ex["voxels"] = sh.deintegrate(fr[p][0], self.depth_source(f, op == "deintegrate_depth"))
            self.count(self.fused, (f, p), -1)
        elif op in ("integrate_color", "integrate_color_map"):
            ex["words"] = sh.integrate_color(fr[f][0], self.depth_source(f, op == "integrate_color"), img, self.band, step["wmax"])
            self.count(self.coloured, (f, f, step["img"]), 1)
        elif op == "deintegrate_color":
            ex["words"] = sh.deintegrate_color(fr[p][0], self.depth_source(f, True), img, self.band)
            self.count(self.coloured, (f, p, step["img"]), -1)
        elif op == "integrate_depth_color":
            ex["words"] = sh.integrate_depth_color(fr[f][0], fr[f][1], fr[f][2], img, self.band, step["wmax"])
            self.count(self.fused, (f, f), 1)
            self.count(self.coloured, (f, f, step["img"]), 1)
        elif op == "deintegrate_depth_color":
            ex["words"] = sh.deintegrate_depth_color(fr[p][0], fr[f][1], img, self.band)
            ex["voxels"] = sh.last_voxels
            self.count(self.fused, (f, p), -1)
            self.count(self.coloured, (f, p, step["img"]), -1)
        elif op == "reintegrate_depth":
            q = step["q"]
            ex["voxels"] = sh.reintegrate_depth(fr[p][0], fr[q][0], fr[f][1], fr[f][2])
            self.count(self.fused, (f, p), -1)
            self.count(self.fused, (f, q), 1)
        elif op == "reintegrate_depth_color":
            q = step["q"]
            ex["words"] = sh.reintegrate_depth_color(fr[p][0], fr[q][0], fr[f][1], fr[f][2], img, self.band, step["wmax"])
            ex["voxels"] = sh.last_voxels
            self.count(self.fused, (f, p), -1)
            self.count(self.fused, (f, q), 1)
            self.count(self.coloured, (f, p, step["img"]), -1)
            self.count(self.coloured, (f, q, step["img"]), 1)
        elif op == "delete_blocks":
            tab = sh.table()
            home = {k: int(h) for k, h in zip(LR.keys_of(tab[tab["ptr"] != -1]), np.nonzero(tab["ptr"] != -1)[0] // sh.params.bucketSize)}
            hashed = LR.MM.hash_block(np.array(step["keys"], np.int64), sh.params.numBuckets).tolist()
            ex["unchained"] = sum(1 for k, h in zip(step["keys"], hashed) if home.get(k, h) != h)
            ex["freed"] = sh.delete_blocks(step["keys"])
        elif op == "garbage_collect":
            ex["listed"] = sh.occupied()
            ex["freed"] = sh.garbage_collect(step["threshold"])
        elif op == "stream_out":
            tab = sh.table().copy()
            chunk = sh.stream_out(step["region"], step["capacity"])
            ex["chunk"], ex["freed"] = chunk, len(chunk["keys"])
            hashed = LR.MM.hash_block(chunk["keys"].astype(np.int64), sh.params.numBuckets).tolist()
            at = {k: i // sh.params.bucketSize for i, k in enumerate(LR.keys_of(tab)) if tab["ptr"][i] != -1}
            ex["unchained"] = sum(1 for k, h in zip(LR.keys_of({"pos": chunk["keys"]}), hashed) if at[k] != h)
            self.store.append({k: chunk[k] for k in ("keys", "voxels", "colors")})
        elif op == "stream_in":
            ex["status"], ex["placed"] = sh.stream_in(step["chunk"])
            ex["present"] = int((ex["status"] == S.PRESENT).sum())
        elif op in ("merge", "merge_color"):
            ex["stats"] = sh.merge(self.src, sh.vs, step["T"], step["mode"], op == "merge_color", step["wmax"])
        elif op == "reload":
            sh.reload(step["with_color"])
        elif op == "clear_color":
            sh.clear_color()
        ex.update(occupied=sh.occupied(), has_color=sh.has_color, live=len(sh.live()), before=before)
        return step


def plan(oracle, variant, sem, seed):
    """The steps of one sequence, each with what the shadow expects of it.  The shadow is advanced as the steps are drawn; a caller
    that needs it (both tests do) builds the Sequence itself and iterates its steps()."""
    return Sequence(oracle, variant, sem, seed).steps()
