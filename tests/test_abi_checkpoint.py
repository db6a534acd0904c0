"""C-ABI checks of the pipeline checkpoint that need no GPU: the new symbols are exported, the ctypes mirrors have the C
layouts, the C digest equals the numpy digest, suma_checkpoint_info parses an image written by checkpoint.py without a
device, checkpoint.py's write -> read round trip is the identity, and the stand-alone parser driver
(tests/cpp/checkpoint_parse_driver.cpp) passes under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_pipeline_checkpoint_size", "suma_pipeline_checkpoint_save", "suma_pipeline_checkpoint_load",
       "suma_checkpoint_info", "suma_checkpoint_params", "suma_checkpoint_digest"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from semantic_suma_amd import core
    return core


def test_new_symbols_are_declared_and_exported(built):
    L = C.CDLL(built.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "suma_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(L, name), name
        assert hasattr(built.lib(), name) and getattr(built.lib(), name).argtypes is not None, name


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import CheckpointInfo, CheckpointSection
    structs = {"suma_checkpoint_section": CheckpointSection, "struct suma_checkpoint_info": CheckpointInfo}
    body = []
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    assert v == want
    assert C.sizeof(CheckpointSection) == 24 and C.sizeof(CheckpointInfo) == 56 + 16 * 24


def test_container_records_match_the_format_header(tmp_path):
    """checkpoint.py's dtypes against csrc/checkpoint_format.h"""
    from semantic_suma_amd import checkpoint as ck
    names = {"Header": ck.HEADER_DTYPE, "DirEntry": ck.DIR_DTYPE, "Pipeline": ck.PIPELINE_DTYPE,
             "MapState": ck.MAP_STATE_DTYPE, "Tile": ck.TILE_DTYPE, "IcpStats": ck.ICP_STATS_DTYPE}
    body = []
    for cname, dt in names.items():
        body.append(f'printf("%zu\\n", sizeof(ckpt::{cname}));')
        body += [f'printf("%zu\\n", offsetof(ckpt::{cname}, {f}));' for f in dt.names]
    src = tmp_path / "fmt.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "checkpoint_format.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "fmt"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "semantic_suma_amd", "csrc"), str(src), "-o",
                           str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for dt in names.values():
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    assert v == want


@pytest.mark.parametrize("nbytes", [0, 8, 64, 4104])
def test_c_digest_equals_numpy(built, nbytes):
    from semantic_suma_amd import checkpoint as ck
    rng = np.random.default_rng(nbytes + 1)
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    got = built.checkpoint_digest(payload)
    assert got == ck.digest(payload)
    # the definition, word by word, in Python integers
    w = np.frombuffer(payload, dtype="<u8")
    want = sum((int(x) + 0x9E3779B97F4A7C15) * (2 * k + 1) for k, x in enumerate(w)) % (1 << 64)
    assert got == want


def minimal_sections(n_active=5, tiles=((0, 1, 3), (2, -1, 4))):
    from semantic_suma_amd import checkpoint as ck
    from semantic_suma_amd.types import SURFEL_DTYPE, default_params
    rng = np.random.default_rng(7)
    T, P = 2, 8
    pipe = np.zeros(1, dtype=ck.PIPELINE_DTYPE)
    pipe["timestamp"] = T
    ms = np.zeros(1, dtype=ck.MAP_STATE_DTYPE)
    ms["timestamp"], ms["n_active"], ms["n_extraction"] = T, n_active, 1
    ext = np.array([[3, -2]], dtype="<i4")
    td = np.zeros(len(tiles), dtype=ck.TILE_DTYPE)
    first = 0
    for k, (i, j, n) in enumerate(tiles):
        td[k] = (i, j, first, n)
        first += n
    rec = lambda n: rng.integers(0, 1 << 32, (n, 16), dtype=np.uint32).view(SURFEL_DTYPE).reshape(-1)
    return dict(
        PARAMS=dict(data=bytes(default_params()), count=1),
        PIPELINE=dict(data=pipe.tobytes(), count=1),
        MAP_STATE=dict(data=ms.tobytes() + ext.tobytes(), count=1),
        POSES=dict(data=rng.random((T, 16), dtype=np.float32).tobytes(), count=T),
        ACTIVE=dict(data=rec(n_active).tobytes(), count=n_active),
        FRAME=dict(data=rng.random((3 * P, 4), dtype=np.float32).tobytes(), count=3 * P),
        TILE_DIR=dict(data=td.tobytes(), count=len(tiles)),
        TILES=dict(data=rec(first).tobytes(), count=first))


def test_info_parses_an_image_written_by_checkpoint_py(built):
    from semantic_suma_amd import checkpoint as ck
    secs = minimal_sections()
    img = ck.write(secs)
    info = built.checkpoint_info(img)
    assert (info["version"], info["timestamp"], info["n_active"], info["n_tiles"], info["n_parked"]) == (1, 2, 5, 2, 7)
    assert (info["has_loop"], info["has_opt"], info["n_nodes"], info["n_edges"]) == (0, 0, 0, 0)
    assert info["total_bytes"] == len(img) and len(img) % 64 == 0
    assert [s["id"] for s in info["sections"]] == list(range(1, 9))
    for s in info["sections"]:
        name = ck.SECTION_NAMES[s["id"]]
        assert s["bytes"] == len(bytes(secs[name]["data"])) and s["digest"] == ck.digest(secs[name]["data"]), name
    assert bytes(built.checkpoint_params(img)) == bytes(secs["PARAMS"]["data"])
    # refused without a device, with a text
    for bad in (img[:-64], img[:10], b"\0" * 128, img[:8] + b"\x07" + img[9:]):
        with pytest.raises(built.SumaError, match="suma_checkpoint_info"):
            built.checkpoint_info(bad)
    overlapping = dict(secs)
    td = np.frombuffer(secs["TILE_DIR"]["data"], dtype=ck.TILE_DTYPE).copy()
    td["first"][1] = 2
    overlapping["TILE_DIR"] = dict(data=td.tobytes(), count=2)
    with pytest.raises(built.SumaError, match="TILE_DIR"):
        built.checkpoint_info(ck.write(overlapping))


def test_write_read_round_trip_is_the_identity():
    from semantic_suma_amd import checkpoint as ck
    secs = minimal_sections()
    img = ck.write(secs)
    back = ck.read(img)
    assert list(back) == list(ck.SECTION_IDS)[:8]
    for k, v in secs.items():
        assert back[k]["data"].tobytes() == bytes(v["data"]) and back[k]["count"] == v["count"], k
    assert ck.verify(img) == []
    assert ck.write(back) == img
    flipped = bytearray(img)
    flipped[len(img) - 100] ^= 1
    assert ck.verify(bytes(flipped)) == ["TILES"]


def test_parser_driver_under_sanitizers(tmp_path):
    """tests/cpp/checkpoint_parse_driver.cpp: a stand-alone program (its own main, only checkpoint_format.h) that runs the
    parser over deterministic mutations of a minimal image, each in a heap block of exactly its length"""
    exe = tmp_path / "parse_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "semantic_suma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "checkpoint_parse_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "mutations" in out.stdout and "accepted" in out.stdout, out.stdout
