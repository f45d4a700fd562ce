"""Connected components of an indexed triangle mesh, restated in NumPy from the rules of include/nfx.h (DESIGN.md section
3.11) — not from the kernel: a sequential union-find over the faces' edges, then label[v] = the smallest vertex index of
v's set.  The yardstick of csrc/mesh_components.hip.  `flood_fill` is a second, independent statement (breadth-first over
an adjacency list) for the small cases."""
import numpy as np


def labels(faces, nv):
    """int32 [nv]: the smallest vertex index of every vertex's component; a vertex that no face names keeps its own."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    assert f.size == 0 or (f.min() >= 0 and f.max() < nv)
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    edges = np.unique(np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]])), axis=1), axis=0)
    for a, b in edges[edges[:, 0] != edges[:, 1]].tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)     # the smaller root stays: a set's root is its minimum
    return np.array([find(v) for v in range(nv)], dtype=np.int32)


def flood_fill(faces, nv):
    """The same labels by breadth-first search from every vertex not yet reached, in ascending order."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    near = [set() for _ in range(nv)]
    for a, b, c in f.tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            if x != y:
                near[x].add(y)
                near[y].add(x)
    out = np.full(nv, -1, dtype=np.int32)
    for start in range(nv):
        if out[start] >= 0:
            continue
        out[start] = start
        front = [start]
        while front:
            nxt = []
            for x in front:
                for y in near[x]:
                    if out[y] < 0:
                        out[y] = start
                        nxt.append(y)
            front = nxt
    return out
