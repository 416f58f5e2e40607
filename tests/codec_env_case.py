"""Subprocess body of test_codec_edges.py's environment-selected forms: the codec with its encode form or grid
forced by the environment (SWARM_ENC_PASSES, SWARM_ENC_PAIR, SWARM_CODEC_WGS, each read once per process),
checked bit-exact against the oracle (agent.py:184-214) on the field and float edges, the tile shapes, the
output placement and the decode layouts.  Prints one JSON line: per case whether it matched and the first
difference."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "distributed-swarm-algorithm_amd")):
    sys.path.insert(0, p)


def main():
    import codec_cases as cc
    from swarm_amd import _lib
    from test_codec_edges import (check_decode, check_encode_decode, check_placement, check_tile_shape,
                                  encode_cases)
    _lib.load()
    cases = []

    def case(name, wide, bad):
        cases.append({"case": name, "wide": wide, "match": not bad, "first_difference": bad[0] if bad else ""})

    shapes = cc.tile_shapes()
    for wide in (False, True):
        for name, cols in encode_cases(wide).items():
            case(name, wide, check_encode_decode(name, cols, wide))
        for name, cols in shapes.items():
            case("tile " + name, wide, check_tile_shape(name, cols, wide))
        case("placement", wide, check_placement(wide))
    for name, (buf, off, _) in cc.decode_layouts().items():
        case("decode " + name, False, check_decode(buf, off, False, 0) + check_decode(buf, off, False, 7, 8))
    return cases


if __name__ == "__main__":
    try:
        cases = main()
        print(json.dumps({"ok": all(c["match"] for c in cases), "cases": cases, "error": ""}))
    except Exception:  # noqa: BLE001 -- reported to the parent test
        print(json.dumps({"ok": False, "cases": [], "error": traceback.format_exc()}))
