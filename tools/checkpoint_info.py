#!/usr/bin/env python3
"""Prints what a pipeline checkpoint file holds (suma_checkpoint_info): needs the built library, no GPU.

    python tools/checkpoint_info.py FILE [--json] [--verify]

--verify also recomputes every payload digest on the host (semantic_suma_amd/checkpoint.py) and names the sections
that differ from the directory."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("file")
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the table")
    ap.add_argument("--verify", action="store_true", help="recompute the payload digests on the host")
    args = ap.parse_args()
    from semantic_suma_amd import checkpoint as ck
    from semantic_suma_amd import core
    img = open(args.file, "rb").read()
    try:
        info = core.checkpoint_info(img)
    except core.SumaError as e:
        print(f"{args.file}: {e}", file=sys.stderr)
        return 1
    bad = ck.verify(img) if args.verify else None
    if args.json:
        print(json.dumps(dict(info, bad_sections=bad)))
        return 1 if bad else 0
    print(f"{args.file}: checkpoint version {info['version']}, {info['total_bytes']} bytes, after {info['timestamp']} scans")
    print(f"  active map {info['n_active']} records; {info['n_tiles']} parked tiles with {info['n_parked']} records")
    print(f"  loop closing {'on' if info['has_loop'] else 'off'}" +
          (f": graph of {info['n_nodes']} nodes, {info['n_edges']} edges" if info["has_loop"] else "") +
          (", an optimisation result waits to be integrated" if info["has_opt"] else ""))
    for s in info["sections"]:
        name = ck.SECTION_NAMES.get(s["id"], "?")
        flag = "" if bad is None else ("  DIGEST MISMATCH" if name in bad else "  ok")
        print(f"  {s['id']:2d} {name:<9s} {s['bytes']:>12d} bytes  digest {s['digest']:016x}{flag}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
