"""The container of a pipeline checkpoint in numpy: image <-> sections, and the digest in ``uint64``.

The image is specified at the top of csrc/k_checkpoint.hip; csrc/checkpoint_format.h holds the C structs this module
mirrors.  ``read`` takes an image apart into its payloads, ``write`` puts payloads together into the canonical image
(offsets, padding, digests, header) -- what tests use to craft and to inspect images, and tools to look into one
without a device.  Nothing here needs the native library.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from .types import CHECKPOINT_MAX_SECTIONS, SURFEL_DTYPE

MAGIC = 0x3150434B414D5553  # the bytes "SUMAKCP1"
VERSION = 1
ALIGN = 64
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
SECTION_IDS = OrderedDict(PARAMS=1, PIPELINE=2, MAP_STATE=3, POSES=4, ACTIVE=5, FRAME=6, TILE_DIR=7, TILES=8, LOOP=9,
                          GRAPH=10, OPT=11)
SECTION_NAMES = {v: k for k, v in SECTION_IDS.items()}

HEADER_DTYPE = np.dtype([("magic", "<u8"), ("version", "<u4"), ("n_sections", "<u4"), ("total_bytes", "<u8")])
DIR_DTYPE = np.dtype([("id", "<u4"), ("reserved", "<u4"), ("offset", "<u8"), ("bytes", "<u8"), ("count", "<u8"),
                      ("digest", "<u8")])
ICP_STATS_DTYPE = np.dtype([("error", "<f8"), ("inlier_residual", "<f8"), ("valid", "<u4"), ("outlier", "<u4"),
                            ("inlier", "<u4"), ("invalid", "<u4"), ("iterations", "<u4"), ("converged", "<u4")])
PIPELINE_DTYPE = np.dtype([("current_pose", "<f8", 16), ("last_pose", "<f8", 16), ("pose_old", "<f8", 16),
                           ("pose_new", "<f8", 16), ("last_increment", "<f8", 16), ("last_pose_old", "<f8", 16),
                           ("timestamp", "<u4"), ("track_loss", "<u4"), ("stats", ICP_STATS_DTYPE),
                           ("stats_mst", ICP_STATS_DTYPE)])
MAP_STATE_DTYPE = np.dtype([("timestamp", "<u4"), ("origin_i", "<i4"), ("origin_j", "<i4"), ("n_active", "<u4"),
                            ("n_updated", "<u4"), ("n_kept_updated", "<u4"), ("n_data", "<u4"), ("n_kept_data", "<u4"),
                            ("n_extraction", "<u4"), ("reserved", "<u4")])
TILE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("first", "<u4"), ("count", "<u4")])
assert (HEADER_DTYPE.itemsize, DIR_DTYPE.itemsize, PIPELINE_DTYPE.itemsize, MAP_STATE_DTYPE.itemsize,
        TILE_DTYPE.itemsize) == (24, 40, 856, 40, 16)


def round_up(v: int) -> int:
    return (v + ALIGN - 1) // ALIGN * ALIGN


def head_bytes(n_sections: int) -> int:
    return round_up(HEADER_DTYPE.itemsize + n_sections * DIR_DTYPE.itemsize + 8)


def digest(payload) -> int:
    """sum over k of (w[k] + 0x9E3779B97F4A7C15) * (2 k + 1) mod 2^64 over the payload's little-endian 64-bit words (a
    shorter tail zero-extended)"""
    b = np.frombuffer(bytes(payload) if not isinstance(payload, np.ndarray) else payload.tobytes(), dtype=np.uint8)
    if len(b) % 8:
        b = np.concatenate([b, np.zeros(8 - len(b) % 8, dtype=np.uint8)])
    w = b.view("<u8")
    k = np.arange(len(w), dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(np.sum((w + GOLDEN) * (k * np.uint64(2) + np.uint64(1)), dtype=np.uint64))


def _payload(data) -> bytes:
    return data.tobytes() if isinstance(data, np.ndarray) else bytes(data)


def read(image) -> "OrderedDict[str, dict]":
    """image -> {section name: {"data": uint8 array (the payload), "count": records, "digest": as the directory states
    it}} in image order.  A helper for tests and tools, not the parser (that is csrc/checkpoint_format.h, behind
    ``core.checkpoint_info``): it checks the magic, the version, the section count, that every id is known and that every
    payload ends inside the image, and raises ValueError otherwise.  It does not check alignment, order or overlap of
    the sections, nor the header's digest, and it does not compare payload digests (``verify`` does)."""
    b = np.frombuffer(bytes(image), dtype=np.uint8)
    if len(b) < HEADER_DTYPE.itemsize:
        raise ValueError("image shorter than its header")
    h = b[:HEADER_DTYPE.itemsize].view(HEADER_DTYPE)[0]
    if int(h["magic"]) != MAGIC or int(h["version"]) != VERSION:
        raise ValueError("not a checkpoint image of this version")
    n = int(h["n_sections"])
    if n > CHECKPOINT_MAX_SECTIONS or head_bytes(n) > len(b):
        raise ValueError("bad directory")
    d = b[HEADER_DTYPE.itemsize:HEADER_DTYPE.itemsize + n * DIR_DTYPE.itemsize].view(DIR_DTYPE)
    out = OrderedDict()
    for e in d:
        off, size = int(e["offset"]), int(e["bytes"])
        if off + size > len(b):
            raise ValueError("section outside the image")
        if int(e["id"]) not in SECTION_NAMES:
            raise ValueError(f"unknown section id {int(e['id'])}")
        out[SECTION_NAMES[int(e["id"])]] = dict(data=b[off:off + size].copy(), count=int(e["count"]),
                                                digest=int(e["digest"]))
    return out


def write(sections) -> bytes:
    """{section name: {"data": array or bytes, "count": records}} -> the canonical image: ascending ids, 64-byte aligned
    zero-padded payloads, digests, header"""
    items = sorted(((SECTION_IDS[k], v) for k, v in sections.items()), key=lambda kv: kv[0])
    n = len(items)
    d = np.zeros(n, dtype=DIR_DTYPE)
    at = head_bytes(n)
    blobs = []
    for k, (sid, v) in enumerate(items):
        p = _payload(v["data"])
        d[k] = (sid, 0, at, len(p), int(v["count"]), digest(p))
        blobs.append((at, p))
        at = round_up(at + len(p))
    img = np.zeros(at, dtype=np.uint8)
    h = np.zeros(1, dtype=HEADER_DTYPE)
    h[0] = (MAGIC, VERSION, n, at)
    head = h.tobytes() + d.tobytes()
    head += np.array([digest(head)], dtype="<u8").tobytes()
    img[:len(head)] = np.frombuffer(head, dtype=np.uint8)
    for off, p in blobs:
        img[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return img.tobytes()


def verify(image) -> list:
    """names of the sections whose payload digest differs from the directory's"""
    return [k for k, v in read(image).items() if digest(v["data"]) != v["digest"]]


def map_state(sections):
    """(the MAP_STATE record, the extraction stack as an (n, 2) int32 array)"""
    raw = sections["MAP_STATE"]["data"]
    return raw[:40].view(MAP_STATE_DTYPE)[0].copy(), raw[40:].view("<i4").reshape(-1, 2).copy()


def with_map(sections, active: np.ndarray, tiles) -> "OrderedDict[str, dict]":
    """a copy of ``sections`` whose active map is ``active`` and whose parked tiles are ``tiles`` ({(i, j): records});
    the last update's counters are cleared"""
    out = OrderedDict((k, dict(v)) for k, v in sections.items())
    ms, ext = map_state(sections)
    ms["n_active"] = len(active)
    ms["n_updated"] = ms["n_kept_updated"] = ms["n_data"] = ms["n_kept_data"] = 0
    out["MAP_STATE"] = dict(data=np.frombuffer(ms.tobytes() + ext.astype("<i4").tobytes(), dtype=np.uint8), count=1)
    out["ACTIVE"] = dict(data=np.ascontiguousarray(active, dtype=SURFEL_DTYPE).view(np.uint8), count=len(active))
    keys = sorted(k for k in tiles if len(tiles[k]))
    td = np.zeros(len(keys), dtype=TILE_DTYPE)
    first = 0
    for n, ij in enumerate(keys):
        td[n] = (ij[0], ij[1], first, len(tiles[ij]))
        first += len(tiles[ij])
    rec = np.concatenate([np.ascontiguousarray(tiles[ij], dtype=SURFEL_DTYPE) for ij in keys]) if keys else \
        np.zeros(0, dtype=SURFEL_DTYPE)
    out["TILE_DIR"] = dict(data=td.view(np.uint8), count=len(keys))
    out["TILES"] = dict(data=rec.view(np.uint8), count=first)
    return out
