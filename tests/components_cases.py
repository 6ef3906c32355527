"""Models chosen for vh_components (the rule: tests/components_ref.py), in tests/mesh_models.py's format, with what the rule
must make of them worked out by hand.  Seeded and pure numpy."""
import itertools

import numpy as np

F = np.float32
OFFSETS = [o for o in itertools.product((0, 1), repeat=3) if o != (0, 0, 0)]                 # (x, y, z): the 7 edges of the rule
ANTI = [(1, -1, 0), (1, 0, -1), (0, 1, -1), (1, 1, -1), (1, -1, 1), (-1, 1, 1)]              # never edges


def index(x, y, z):
    return ((z & 7) << 6) | ((y & 7) << 3) | (x & 7)


def signs(outside):
    """(sdf of a node of the pair / the path, sdf of the rest) for the target: inside nodes in an outside sea, or swapped."""
    return (F(1.0), F(-1.0)) if outside else (F(-1.0), F(1.0))


def offsets(outside=False):
    """One model with, for each of the 7 offsets o and each of the 6 anti-offsets, a pair {A, A + o} of the target class in a
    sea of the other class: once inside a block and once across every seam the offset can cross (every non-empty subset of
    its non-zero axes), with only the blocks of A and of A + o present -- so for (1, 1, 1) across the corner only the corner
    neighbour is there.  The pairs lie three blocks apart.  Returns (model, pairs); a pair is a dict of A, B (global voxels),
    o, cross (the axes crossed) and the expectation: joined6, joined14."""
    node, sea = signs(outside)
    model, pairs = {}, []
    for o in OFFSETS + ANTI:
        axes = [a for a in range(3) if o[a]]
        for r in range(len(axes) + 1):
            for cross in itertools.combinations(axes, r):
                n = len(pairs)
                base = np.array((3 * (n % 8) - 11, 3 * ((n // 8) % 4) - 5, 3 * (n // 32) - 2))
                local = np.array([(7 if o[a] > 0 else 0) if a in cross else 3 for a in range(3)])
                A = base * 8 + local
                B = A + np.array(o)
                for g in (A, B):
                    k = tuple(int(c) >> 3 for c in g)
                    if k not in model:
                        model[k] = (np.full(512, sea, F), np.ones(512, F))
                    model[k][0][index(*(int(c) for c in g))] = node
                assert (tuple(int(c) >> 3 for c in A) != tuple(int(c) >> 3 for c in B)) == bool(cross)
                is_edge = o in OFFSETS
                pairs.append(dict(A=tuple(int(c) for c in A), B=tuple(int(c) for c in B), o=o, cross=cross,
                                  joined6=is_edge and sum(o) == 1, joined14=is_edge))
    return model, pairs


SERPENTINE_NODES, SERPENTINE_REST = 609, 36 * 512 - 609


def serpentine(outside=False):
    """6 x 6 x 1 blocks of the sea, one path of 609 nodes at z = 3: the rows y = 1, 5, ..., 45 over x = 0 .. 47, joined at
    alternate ends by the three voxels between them.  One component of 609 nodes in all 36 blocks at 6 and at 14; the rest
    (17 823 voxels) is one component of the other class at 6."""
    node, sea = signs(outside)
    model = {(x, y, 0): (np.full(512, sea, F), np.ones(512, F)) for y in range(6) for x in range(6)}
    path = []
    rows = list(range(1, 48, 4))
    for i, y in enumerate(rows):
        path += [(x, y) for x in range(48)]
        if i + 1 < len(rows):
            x = 47 if i % 2 == 0 else 0
            path += [(x, y + d) for d in (1, 2, 3)]
    assert len(set(path)) == len(path) == SERPENTINE_NODES
    for x, y in path:
        model[(x >> 3, y >> 3, 0)][0][index(x, y, 3)] = node
    return model


def sparse(p, seed=31):
    """About 80 % of the 4 x 3 x 3 keys around (-2, 1, -1); a voxel is inside with probability p, 5 % of the weights are 0."""
    rng = np.random.RandomState(seed)
    model = {}
    for z, y, x in itertools.product(range(-2, 1), range(0, 3), range(-4, 0)):
        if rng.uniform() < 0.8:
            sdf = np.where(rng.uniform(size=512) < p, F(-1.0), F(1.0)).astype(F) * rng.uniform(0.1, 1.0, 512).astype(F)
            model[(x, y, z)] = (sdf.astype(F), np.where(rng.uniform(size=512) < 0.05, 0, 1).astype(F))
    return model
