"""Writers for the surface mesh (include/dedflow.h, "surface mesh"): binary little-endian PLY with per-vertex scalar properties,
and binary STL.  Pure numpy.  The readers read back exactly what the writers wrote and serve the tests."""
import numpy as np


def _arrays(verts, tris):
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    if tris.size and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError("a triangle refers to a vertex outside the list")
    return verts, tris


def write_ply(path, verts, tris, fields=None, names=None):
    """verts [nv, 3] float64, tris [nt, 3] int32, fields [nv, K] float64 (or None) as the vertex properties `names` (default
    f0, f1, ...): the doubles are written as they are, so a round trip returns the same bits"""
    verts, tris = _arrays(verts, tris)
    nv = len(verts)
    fields = np.zeros((nv, 0)) if fields is None else np.ascontiguousarray(fields, np.float64)
    if fields.ndim != 2 or len(fields) != nv:
        raise ValueError("fields must be [%d, K]" % nv)
    K = fields.shape[1]
    names = ["f%d" % k for k in range(K)] if names is None else list(names)
    if len(names) != K or len(set(names) | {"x", "y", "z"}) != K + 3 or any(not n or not n.isidentifier() for n in names):
        raise ValueError("names must be %d distinct identifiers other than x, y, z" % K)
    head = ["ply", "format binary_little_endian 1.0", "comment dedflow surface mesh", "element vertex %d" % nv]
    head += ["property double %s" % n for n in ["x", "y", "z"] + names]
    head += ["element face %d" % len(tris), "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(nv, np.dtype([(n, "<f8") for n in ["x", "y", "z"] + names]))
    for d, n in enumerate("xyz"):
        vrec[n] = verts[:, d]
    for k, n in enumerate(names):
        vrec[n] = fields[:, k]
    frec = np.empty(len(tris), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    frec["n"] = 3
    frec["v"] = tris
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    """(verts, tris, fields, names) of a file write_ply wrote"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    nv = nt = 0
    props = []
    for ln in lines:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nt = int(w[2])
        elif w[:2] == ["property", "double"]:
            props.append(w[2])
    vdt = np.dtype([(n, "<f8") for n in props])
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    vrec = np.frombuffer(data, vdt, nv, end)
    frec = np.frombuffer(data, fdt, nt, end + nv * vdt.itemsize)
    names = props[3:]
    verts = np.stack([vrec[n] for n in "xyz"], axis=1) if nv else np.zeros((0, 3))
    fields = np.stack([vrec[n] for n in names], axis=1) if names and nv else np.zeros((nv, len(names)))
    return verts, frec["v"].astype(np.int32).reshape(-1, 3), fields, names


_STL = np.dtype([("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])


def write_stl(path, verts, tris):
    """binary STL: float32 corners in the triangle's own order; the facet normal is the unit vector of its own cross product
    (B - A) x (C - A), formed in float64 from the float64 corners; a zero-area triangle is kept with a zero normal"""
    verts, tris = _arrays(verts, tris)
    P = verts[tris]                                                          # [nt, 3, 3]
    rec = np.zeros(len(tris), _STL)
    if len(tris):
        n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        ln = np.sqrt((n * n).sum(axis=1))
        ok = np.isfinite(ln) & (ln > 0)
        n[ok] /= ln[ok, None]
        n[~ok] = 0.0
        rec["n"] = n
        rec["v"] = P
    with open(path, "wb") as fh:
        fh.write(b"dedflow surface mesh".ljust(80, b" "))
        fh.write(np.array([len(tris)], "<u4").tobytes())
        fh.write(rec.tobytes())


def read_stl(path):
    """(corners [nt, 3, 3] float32, normals [nt, 3] float32) of a binary STL"""
    with open(path, "rb") as fh:
        data = fh.read()
    nt = int(np.frombuffer(data, "<u4", 1, 80)[0])
    if len(data) != 84 + nt * _STL.itemsize:
        raise ValueError("not a binary STL: %d bytes for %d facets" % (len(data), nt))
    rec = np.frombuffer(data, _STL, nt, 84)
    return rec["v"].copy(), rec["n"].copy()
