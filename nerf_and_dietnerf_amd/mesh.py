"""Triangle meshes on disk: binary little-endian PLY, the layout NeRF.extract_mesh writes.

Per vertex: float x y z, then (with normals) float nx ny nz, then (with colours) uchar red green blue; per face a
``uchar int`` list (always 3 indices here).  ``read_ply`` reads what ``write_ply`` writes, not PLY in general.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

_HEAD = b"ply\nformat binary_little_endian 1.0\n"


def _colors_u8(colors) -> np.ndarray:
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        return c
    return np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)      # [0, 1] floats


def write_ply(path, vertices, triangles, normals=None, colors=None) -> None:
    """``vertices`` (V, 3) and ``normals`` (V, 3) float32, ``colors`` (V, 3) uint8 or floats in [0, 1], ``triangles`` (T, 3)
    int32 indices into the vertices."""
    v = np.asarray(vertices, "<f4")
    t = np.asarray(triangles, "<i4")
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"vertices must be (V, 3) and triangles (T, 3), got {v.shape} and {t.shape}")
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle index is outside the vertex array")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.zeros(len(v), dtype=fields)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    for name, block, keys in (("normals", normals, ("nx", "ny", "nz")), ("colors", colors, ("red", "green", "blue"))):
        if block is None:
            continue
        b = _colors_u8(block) if name == "colors" else np.asarray(block, "<f4")
        if b.shape != v.shape:
            raise ValueError(f"{name} must be {v.shape}, got {b.shape}")
        for i, k in enumerate(keys):
            rec[k] = b[:, i]
    faces = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"], faces["i"] = 3, t
    head = _HEAD + f"element vertex {len(v)}\n".encode()
    for k, ty in fields:
        head += f"property {'float' if ty == '<f4' else 'uchar'} {k}\n".encode()
    head += f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n".encode()
    with open(path, "wb") as f:
        f.write(head)
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def read_ply(path) -> Dict[str, Optional[np.ndarray]]:
    """-> {"vertices", "triangles", "normals" (or None), "colors" (uint8, or None)} of a file write_ply wrote."""
    with open(path, "rb") as f:
        data = f.read()
    if not data.startswith(_HEAD):
        raise ValueError(f"{path}: not a binary little-endian PLY")
    end = data.index(b"end_header\n") + len(b"end_header\n")
    counts, fields, element = {}, [], None
    for line in data[len(_HEAD):end].decode("ascii").splitlines():
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
            counts[element] = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            if w[1] not in ("float", "uchar"):
                raise ValueError(f"{path}: vertex property type {w[1]!r} is not one write_ply writes")
            fields.append((w[2], "<f4" if w[1] == "float" else "u1"))
        elif w[:1] == ["property"] and element == "face" and w[1:4] != ["list", "uchar", "int"]:
            raise ValueError(f"{path}: faces are not uchar/int lists")
    nv, nt = counts.get("vertex", 0), counts.get("face", 0)
    vdt = np.dtype(fields)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(data) != end + nv * vdt.itemsize + nt * fdt.itemsize:
        raise ValueError(f"{path}: size does not match the header (only triangles are supported)")
    rec = np.frombuffer(data, vdt, nv, end)
    faces = np.frombuffer(data, fdt, nt, end + nv * vdt.itemsize)
    if nt and (faces["n"] != 3).any():
        raise ValueError(f"{path}: a face is not a triangle")
    names = [k for k, _ in fields]

    def block(keys, dtype):
        return np.stack([rec[k] for k in keys], axis=1).astype(dtype) if all(k in names for k in keys) else None
    return {"vertices": block(("x", "y", "z"), np.float32), "triangles": faces["i"].astype(np.int32).reshape(nt, 3),
            "normals": block(("nx", "ny", "nz"), np.float32), "colors": block(("red", "green", "blue"), np.uint8)}
