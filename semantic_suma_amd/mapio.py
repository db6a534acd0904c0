"""Files of an exported map: SurfelMap.export_world's records as a binary little-endian PLY point cloud.

    write_ply(path, world_surfels, color_map=None)   x y z nx ny nz radius confidence label prob support + red green blue
    read_ply(path) -> (world_surfels, rgb)           the round trip (timestamp, which the file does not carry, reads 0)

and core.world_grid's traversability grid as one .npz:

    write_grid(path, cells, params)                  the cells [height, width] and the GridParams that made them
    read_grid(path) -> (cells, params)

and core.grid_plan's field beside it:

    write_plan(path, field, grid_params, plan_params)   the field [height, width] and both parameter structs
    read_plan(path) -> (field, grid_params, plan_params)
"""
from __future__ import annotations

import numpy as np

from . import kitti
from .types import GRID_CELL_DTYPE, PLAN_CELL_DTYPE, WORLD_SURFEL_DTYPE, GridParams, PlanParams

# the PLY vertex: name, PLY type, numpy type
_PLY_FIELDS = [("x", "float", "<f4"), ("y", "float", "<f4"), ("z", "float", "<f4"),
               ("nx", "float", "<f4"), ("ny", "float", "<f4"), ("nz", "float", "<f4"),
               ("radius", "float", "<f4"), ("confidence", "float", "<f4"), ("label", "uint", "<u4"),
               ("prob", "float", "<f4"), ("support", "uint", "<u4"),
               ("red", "uchar", "u1"), ("green", "uchar", "u1"), ("blue", "uchar", "u1")]
_PLY_DTYPE = np.dtype([(n, t) for n, _, t in _PLY_FIELDS])
_PLY_NP = {"float": "<f4", "float32": "<f4", "uint": "<u4", "uint32": "<u4", "uchar": "u1", "uint8": "u1",
           "int": "<i4", "int32": "<i4", "double": "<f8", "float64": "<f8", "ushort": "<u2", "uint16": "<u2",
           "short": "<i2", "int16": "<i2", "char": "i1", "int8": "i1"}


def write_ply(path: str, world_surfels: np.ndarray, color_map=None) -> None:
    """``world_surfels``: WORLD_SURFEL_DTYPE records; ``color_map``: uint8 [260, 3] RGB by label id (default
    kitti.semantic_color_map()); a label outside the map is black"""
    ws = np.ascontiguousarray(world_surfels, dtype=WORLD_SURFEL_DTYPE)
    cmap = np.asarray(kitti.semantic_color_map() if color_map is None else color_map, dtype=np.uint8).reshape(-1, 3)
    v = np.zeros(ws.shape[0], dtype=_PLY_DTYPE)
    for name, _, _ in _PLY_FIELDS[:-3]:
        v[name] = ws[name]
    inside = ws["label"] < cmap.shape[0]
    rgb = np.where(inside[:, None], cmap[np.where(inside, ws["label"], 0)], 0).astype(np.uint8)
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ["ply", "format binary_little_endian 1.0", "comment semantic surfel map, world frame",
              f"element vertex {ws.shape[0]}"]
    header += [f"property {t} {n}" for n, t, _ in _PLY_FIELDS] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(v.tobytes())


def read_ply(path: str):
    """-> (WORLD_SURFEL_DTYPE records, uint8 [n, 3] RGB) of a binary little-endian PLY whose vertex element holds scalar
    properties (any order; those write_ply does not know are skipped, those missing read 0)"""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        n, props, in_vertex, fmt = 0, [], False, None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            w = line.decode("ascii").split()
            if not w or w[0] == "comment":
                continue
            if w[0] == "end_header":
                break
            if w[0] == "format":
                fmt = w[1]
            elif w[0] == "element":
                in_vertex = w[1] == "vertex"
                if in_vertex:
                    n = int(w[2])
                elif not props:
                    raise ValueError(f"{path}: element {w[1]} in front of the vertices")
            elif w[0] == "property" and in_vertex:
                if w[1] == "list" or w[1] not in _PLY_NP:
                    raise ValueError(f"{path}: vertex property {' '.join(w[1:])} is not a known scalar")
                props.append((w[2], _PLY_NP[w[1]]))
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: format {fmt!r} (only binary_little_endian is read)")
        dt = np.dtype(props)
        v = np.frombuffer(f.read(n * dt.itemsize), dtype=dt)
    if v.shape[0] != n:
        raise ValueError(f"{path}: {v.shape[0]} of {n} vertices")
    ws = np.zeros(n, dtype=WORLD_SURFEL_DTYPE)
    for name in WORLD_SURFEL_DTYPE.names:
        if name in dt.names:
            ws[name] = v[name]
    rgb = np.zeros((n, 3), dtype=np.uint8)
    for k, name in enumerate(("red", "green", "blue")):
        if name in dt.names:
            rgb[:, k] = v[name]
    return ws, rgb


def write_grid(path: str, cells: np.ndarray, params: GridParams) -> None:
    """``cells``: GRID_CELL_DTYPE [height, width] as core.world_grid returns them; ``params``: the GridParams of that call
    (cell size, origin and size place the raster in the world frame).  ``path`` is written as given (end it in .npz)."""
    c = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE)
    if c.shape != (params.height, params.width):
        raise ValueError(f"write_grid: cells {c.shape} against a raster of {params.height} x {params.width}")
    with open(path, "wb") as f:
        np.savez_compressed(f, cells=c.view(np.uint8).reshape(c.shape + (GRID_CELL_DTYPE.itemsize,)),
                            params=np.frombuffer(bytes(params), dtype=np.uint8))


def read_grid(path: str):
    """-> (GRID_CELL_DTYPE cells [height, width], GridParams) of a file write_grid made"""
    with np.load(path) as z:
        raw, par = z["cells"], z["params"]
    if par.dtype != np.uint8 or par.size != len(bytes(GridParams())) or raw.dtype != np.uint8 or raw.ndim != 3 or \
            raw.shape[2] != GRID_CELL_DTYPE.itemsize:
        raise ValueError(f"{path}: not a grid file")
    gp = GridParams.from_buffer_copy(par.tobytes())
    if raw.shape[:2] != (gp.height, gp.width):
        raise ValueError(f"{path}: cells {raw.shape[:2]} against a raster of {gp.height} x {gp.width}")
    return np.ascontiguousarray(raw).view(GRID_CELL_DTYPE).reshape(gp.height, gp.width), gp


def write_plan(path: str, field: np.ndarray, grid_params: GridParams, plan_params: PlanParams) -> None:
    """``field``: PLAN_CELL_DTYPE [height, width] as core.grid_plan returns it, with the GridParams of the grid it was
    planned on and the PlanParams of that call.  ``path`` is written as given (end it in .npz)."""
    f_ = np.ascontiguousarray(field, dtype=PLAN_CELL_DTYPE)
    if f_.shape != (grid_params.height, grid_params.width):
        raise ValueError(f"write_plan: field {f_.shape} against a raster of {grid_params.height} x {grid_params.width}")
    with open(path, "wb") as f:
        np.savez_compressed(f, field=f_.view(np.uint8).reshape(f_.shape + (PLAN_CELL_DTYPE.itemsize,)),
                            params=np.frombuffer(bytes(grid_params), dtype=np.uint8),
                            plan_params=np.frombuffer(bytes(plan_params), dtype=np.uint8))


def read_plan(path: str):
    """-> (PLAN_CELL_DTYPE field [height, width], GridParams, PlanParams) of a file write_plan made"""
    with np.load(path) as z:
        if not {"field", "params", "plan_params"} <= set(z.files):
            raise ValueError(f"{path}: not a plan file")
        raw, par, ppar = z["field"], z["params"], z["plan_params"]
    if par.dtype != np.uint8 or par.size != len(bytes(GridParams())) or ppar.dtype != np.uint8 or \
            ppar.size != len(bytes(PlanParams())) or raw.dtype != np.uint8 or raw.ndim != 3 or \
            raw.shape[2] != PLAN_CELL_DTYPE.itemsize:
        raise ValueError(f"{path}: not a plan file")
    gp = GridParams.from_buffer_copy(par.tobytes())
    if raw.shape[:2] != (gp.height, gp.width):
        raise ValueError(f"{path}: field {raw.shape[:2]} against a raster of {gp.height} x {gp.width}")
    return (np.ascontiguousarray(raw).view(PLAN_CELL_DTYPE).reshape(gp.height, gp.width), gp,
            PlanParams.from_buffer_copy(ppar.tobytes()))
