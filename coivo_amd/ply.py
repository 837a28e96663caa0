"""write_ply: a cloud or a mesh as a binary PLY file.  Host code.  coivo_amd.inference re-exports it."""
from typing import Optional

import torch


def write_ply(path, points: torch.Tensor, colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
              faces: Optional[torch.Tensor] = None) -> None:
    """Binary little-endian PLY: `float x y z` per vertex, with normals [M,3] `float nx ny nz` behind them (viewers shade by them)
    and, with colours [M,3] in [0,1], `uchar red green blue` (rint(c * 255), clamped).  With faces [F,3] (integer vertex indices, a
    Mesh's `faces`) an `element face F` with `property list uchar int vertex_indices` follows the vertices.  Without normals and
    without faces the bytes are what they were before either existed.  Host code; one device -> host copy (two with faces)."""
    import numpy as np
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("write_ply: points must be [M,3]")
    if faces is not None:
        if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point()
                or faces.dtype == torch.bool):
            raise ValueError("write_ply: faces must be an integer tensor [F,3]")
        if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= points.shape[0]):
            raise ValueError("write_ply: faces index vertices that do not exist")
    if colors is not None and tuple(colors.shape) != tuple(points.shape):
        raise ValueError("write_ply: colors must have the shape of points")
    if normals is not None and (not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape)):
        raise ValueError("write_ply: normals must be a tensor of the shape of points")
    parts = [points.detach().to(torch.float32)]
    if normals is not None:
        parts.append(normals.detach().to(points.device, torch.float32))
    if colors is not None:
        parts.append(colors.detach().to(points.device, torch.float32))
    host = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)).cpu().numpy()
    m = host.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {m}", "property float x", "property float y",
              "property float z"]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    if faces is not None:
        header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices"]
    header.append("end_header")
    rows = np.empty(m, dtype=np.dtype(fields))
    n_float = 3 if normals is None else 6
    for a, name in enumerate(("x", "y", "z", "nx", "ny", "nz")[:n_float]):
        rows[name] = host[:, a]
    if colors is not None:
        q = np.clip(np.rint(np.nan_to_num(host[:, n_float:n_float + 3], nan=0.0) * 255.0), 0, 255).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            rows[name] = q[:, k]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rows.tobytes())
        if faces is not None:
            tri = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            tri["n"] = 3
            tri["v"] = faces.detach().cpu().numpy()
            f.write(tri.tobytes())
