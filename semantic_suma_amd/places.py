"""A place index with the poses of its entries in one file: ``save(path, index, poses)`` / ``load(path)``.

The file is one ``.npz`` with the descriptor parameters (rings, sectors, max_range, height_offset, keep_label), the cells
(n x sectors x rings, fp32), the ids and one row-major 4x4 pose per entry.  The norms are not stored: the library makes
them on the device from the cells (core.PlaceIndex.upload).  tools/export_map.py --places writes such a file beside the
map, tools/localize.py --relocalize reads it."""
from __future__ import annotations

import numpy as np

from . import core
from .types import DRAW_COLORS, PlaceParams

FORMAT_VERSION = 1


def save(path: str, index: "core.PlaceIndex", poses) -> None:
    """``poses``: one 4x4 pose per entry, by entry index (the session's final trajectory)"""
    cells, _, ids = index.download()
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if poses.shape[0] != cells.shape[0]:
        raise ValueError(f"{poses.shape[0]} poses for {cells.shape[0]} entries")
    p = index.params
    with open(path, "wb") as f:  # a file object: numpy adds no suffix to the name
        np.savez(f, version=np.uint32(FORMAT_VERSION), rings=np.uint32(p.rings), sectors=np.uint32(p.sectors),
                 max_range=np.float32(p.max_range), height_offset=np.float32(p.height_offset),
                 keep_label=np.frombuffer(bytes(p.keep_label), dtype=np.uint8).copy(), cells=cells, ids=ids, poses=poses)


def load(path: str, device: int = 0):
    """-> (core.PlaceIndex, poses n x 4 x 4)"""
    with np.load(path) as z:
        if int(z["version"]) != FORMAT_VERSION:
            raise ValueError(f"{path}: format version {int(z['version'])}, expected {FORMAT_VERSION}")
        keep = np.asarray(z["keep_label"], dtype=np.uint8)
        if keep.shape != (DRAW_COLORS,):
            raise ValueError(f"{path}: keep_label has {keep.shape} entries")
        p = PlaceParams.defaults(keep_labels=np.nonzero(keep)[0], rings=int(z["rings"]), sectors=int(z["sectors"]),
                                 max_range=float(z["max_range"]), height_offset=float(z["height_offset"]))
        cells, ids, poses = z["cells"], z["ids"], np.asarray(z["poses"], dtype=np.float64)
    if cells.shape != (ids.shape[0], p.sectors, p.rings) or poses.shape != (ids.shape[0], 4, 4):
        raise ValueError(f"{path}: cells {cells.shape}, ids {ids.shape} and poses {poses.shape} do not fit")
    index = core.PlaceIndex(p, device=device, capacity=ids.shape[0])
    if ids.shape[0]:
        index.upload(cells, ids)
    return index, poses
