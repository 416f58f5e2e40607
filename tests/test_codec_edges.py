"""The wire codec where its kernels branch (cases: tests/codec_cases.py).

tests/test_codec.py pins the codec to the reference's known answers and to random batches.  Here every
comparison is bit-exact against the struct restatement of agent.py:184-214 (oracle.codec_*_py; floats as
uint32 views, so a NaN's payload and the sign of zero count), on cases built for the places where
csrc/codec.hip takes another path:
  fields      every integer field at the edges of u8 / u32 / int64; types that are 1..5 only modulo 2^8 or
              2^32 (unknown to the reference: status 3); floats at +-0, inf, NaNs with payloads, the f32
              subnormal edge and both sides of the rounding midpoint above FLT_MAX
  tiles       message counts around the 2 048-message encode tile, a look-back over more than 64 tiles, tiles
              of zero bytes, of under 16 bytes (no 16-byte store), of 17-byte packets only (a full LDS buffer)
  placement   `out` at each of the 16 byte phases inside a larger buffer: the bytes, and nothing outside them;
              cap == total, and caps that are too small (SWARM_ERR_RANGE, nothing at or past out + cap)
  arrays      status / offsets / one input column alone off its 16-byte alignment
  decode      every type byte at every length, NaN payloads, chunk sizes around 1 024 packets, a chunk too
              large to stage, offsets that lie inside a chunk whose endpoints are fine; `buf` at byte phases
              that take the staged and the global path
  forms       the three-pass encode, one message per lane, one workgroup for everything: child processes
The CPU tests pin the cases themselves, so an edit to the builders cannot hollow out the GPU tests.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import codec_cases as cc
from oracle import oracle

DEC_KEYS = ("status", "type", "sender", "tick", "task", "winner", "has_pos", "a", "b")
PAD = 64  # guard bytes on either side of an output view (a multiple of 16)
# the cases the GPU tests are parametrised over, by name (the CPU tests check that none is left out)
TILE_NAMES = ["m1", "m2", "m3", "m2047", "m2048", "m2049", "m4097", "m6145", "m133121", "error_tile_between",
              "one_coordinator_tile", "first_tile_errors", "conflict_tile"]
LAYOUT_NAMES = ["m1", "m1023", "m1024", "m1025", "m2049", "m3073", "short_last_chunk", "oversized_packet",
                "bad_offsets"]
_WANT = {}


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def first_diff(name, got, want):
    """None, or where two arrays first differ (floats by bit pattern)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind == "f" or want.dtype.kind == "f":
        got, want = bits(got), bits(want)
    if got.shape != want.shape:
        return "%s: shape %s, want %s" % (name, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        return "%s[%d]: got %s, want %s (%d differ)" % (name, i, got[i], want[i], bad.size)
    return None


def want_encode(key, cols, wide):
    """The oracle's framing of a case, computed once per (case, wide) and shared."""
    if (key, wide) not in _WANT:
        st, pk = oracle.codec_encode_py(*cols, wide=wide)
        off = np.concatenate([[0], np.cumsum([len(p) for p in pk])]).astype(np.int64)
        w = dict(status=st, packets=pk, offsets=off, buf=np.frombuffer(b"".join(pk), np.uint8), total=int(off[-1]))
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[key, wide] = w
    return _WANT[key, wide]


def want_decode(buf, off, wide):
    """Status 4 (fields 0) for a packet whose offsets leave [0, len(buf)] or run backwards; every other packet
    as the oracle parses buf[off[i]:off[i+1]]."""
    raw, pb, pe = bytes(buf), off[:-1], off[1:]
    inside = (0 <= pb) & (pb <= pe) & (pe <= len(raw))
    d = oracle.codec_decode_py([raw[pb[i]:pe[i]] if inside[i] else b"" for i in range(len(pb))], wide=wide)
    d["status"] = np.where(inside, d["status"], 4)
    return d, inside


def encode_cases(wide):
    return {"field_edges": cc.field_edges(wide), "float_edges": cc.float_edges()}


# ----------------------------------------------------------------------------- CPU: the cases themselves

@pytest.mark.parametrize("wide", [False, True])
def test_every_status_occurs_for_every_type_it_can(wide):
    cols = cc._cat(cc.field_edges(wide), cc.float_edges())
    st = want_encode("all_edges", cols, wide)["status"]
    seen = {(int(t), int(s)) for t, s in zip(cols[0], st) if 1 <= t <= 5}
    assert seen == {(t, s) for t in cc.TYPES for s in (0, 1)} | {(cc.HB, 2), (cc.CLAIM, 2)}
    unknown = ~np.isin(cols[0], cc.TYPES)
    assert set(cols[0][unknown]) == set(cc.EDGE_TYPES) and (st[unknown] == 3).all() and (st[~unknown] != 3).all()
    # each field's range is met from both sides: 255 | 256 (u8 IDs), 2^32-1 | 2^32, 0 | -1
    id_top = 2**32 - 1 if wide else 255
    f = cc.field_edges(wide)
    fst = want_encode("field_edges", f, wide)["status"]
    for ty, col, top in ((cc.ACCLAIM, 1, id_top), (cc.COORD, 2, 2**32 - 1), (cc.CLAIM, 5, 2**32 - 1),
                         (cc.CONFLICT, 6, id_top), (cc.HB, 1, id_top)):
        sel = f[0] == ty
        for v, s in ((top, 0), (top + 1, 1), (0, 0), (-1, 1), (2**63 - 1, 1), (-2**63, 1)):
            hit = sel & (f[col] == v)
            assert hit.any() and (fst[hit] == s).all(), (ty, col, v)


def test_types_valid_only_modulo_a_power_of_two_are_unknown():
    ty = np.array([2**32 + 3, 2**32 + 1, -2**32 + 3, 257] + [2**32 + k for k in range(1, 6)] +
                  [-2**32 + k for k in range(1, 6)] + [256 + k for k in range(1, 6)], np.int64)
    assert set((ty % 256).tolist()) == {1, 2, 3, 4, 5} and set(ty[:14].tolist()) <= set(cc.EDGE_TYPES)
    rows = cc._cols([dict(cc.BASE, type=int(t)) for t in ty])
    for wide in (False, True):
        st, pk = oracle.codec_encode_py(*rows, wide=wide)
        assert st.tolist() == [3] * len(ty) and not any(pk)


def test_both_sides_of_the_f32_midpoint():
    mid, below, above = cc.F32_MIDPOINT, np.nextafter(cc.F32_MIDPOINT, 0.0), np.nextafter(cc.F32_MIDPOINT, np.inf)
    assert below < mid < above and {mid, below, above, -mid, -below, -above} <= set(cc.FLOAT_EDGES)
    for sign in (1.0, -1.0):
        rows = cc._cols([dict(cc.BASE, type=t, a=sign * v) for t in (cc.HB, cc.CLAIM) for v in (below, mid, above)])
        st, pk = oracle.codec_encode_py(*rows)
        assert st.tolist() == [0, 2, 2, 0, 2, 2]
        flt_max = (0x7F7FFFFF | (0x80000000 if sign < 0 else 0)).to_bytes(4, "big")
        assert pk[0][6:10] == flt_max and pk[3][10:14] == flt_max


def test_float_edges_hold_what_they_promise():
    b = np.array(cc.FLOAT_EDGES, np.float64).view(np.uint64)
    nan = np.isnan(cc.FLOAT_EDGES)
    assert {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000,
            0xFFF8000000000000} <= set(b.tolist())
    mant = b[nan] & ((1 << 52) - 1)
    assert ((mant >> 29) & 0x3FFFFF).any() and ((mant >> 29 == 1 << 22) & ((mant & 0x1FFFFFFF) != 0)).any()
    assert ((mant >> 51) == 0).any() and ((mant >> 29 == 0) & (mant != 0)).any()   # signalling; low bits only
    assert {2.0**-149, 2.0**-150, -2.0**-149, -2.0**-150, cc.FLT_MAX, -cc.FLT_MAX} <= set(cc.FLOAT_EDGES)
    st = want_encode("float_edges", cc.float_edges(), False)["status"]
    assert {0, 2} == set(st.tolist())


@pytest.mark.parametrize("wide", [False, True])
def test_oracle_round_trip_returns_every_field(wide):
    for name, cols in encode_cases(wide).items():
        w = want_encode(name, cols, wide)
        ok = w["status"] == 0
        assert ok.any()
        d = oracle.codec_decode_py([p for p in w["packets"] if p], wide=wide)
        assert (d["status"] == 0).all()
        ty = cols[0][ok]
        with np.errstate(invalid="ignore", over="ignore"):  # (a claim's b may be anything: it is not framed)
            a32, b32 = bits(cols[3][ok].astype(np.float32)), bits(cols[4][ok].astype(np.float32))
        hb, cl, cf = ty == cc.HB, ty == cc.CLAIM, ty == cc.CONFLICT
        for k, v in (("type", ty), ("sender", cols[1][ok]), ("tick", cols[2][ok])):
            np.testing.assert_array_equal(d[k], v, err_msg=k)
        np.testing.assert_array_equal(d["has_pos"], hb)
        np.testing.assert_array_equal(bits(d["a"]), np.where(hb | cl, a32, 0), err_msg="a")
        np.testing.assert_array_equal(bits(d["b"]), np.where(hb, b32, 0), err_msg="b")
        np.testing.assert_array_equal(d["task"], np.where(cl | cf, cols[5][ok], 0))
        np.testing.assert_array_equal(d["winner"], np.where(cf, cols[6][ok], 0))


def test_tile_shapes_are_the_tiles_they_claim():
    shapes = cc.tile_shapes()
    T = cc.TILE
    assert sorted(shapes) == sorted(TILE_NAMES)
    assert [len(shapes["m%d" % m][0]) for m in (1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1, 65 * T + 1)] == \
        [1, 2, 3, 2047, 2048, 2049, 4097, 6145, 133121]
    assert max(len(c[0]) for c in shapes.values()) <= 135_000
    for wide in (False, True):
        tile_bytes = {k: np.add.reduceat(np.diff(want_encode(k, c, wide)["offsets"]), np.arange(0, len(c[0]), T))
                      for k, c in shapes.items() if not k.startswith("m")}
        assert tile_bytes["error_tile_between"][1] == 0 and tile_bytes["error_tile_between"][[0, 2]].min() > 16
        assert tile_bytes["one_coordinator_tile"][1] == (9 if wide else 6)
        assert tile_bytes["first_tile_errors"][0] == 0 and tile_bytes["first_tile_errors"][1] > 16
        assert tile_bytes["conflict_tile"][1] == T * (17 if wide else 11)
        assert tile_bytes["conflict_tile"][0] % 4 != 0   # the full tile is stored shifted, not at phase 0
        for k in ("m%d" % (3 * T + 1), "m%d" % (65 * T + 1)):
            assert {0, 1, 2, 3} <= set(want_encode(k, shapes[k], wide)["status"].tolist())
    w = want_encode("placement", cc.placement_batch(), False)
    assert len(w["status"]) > 2 * T and {0, 1, 2, 3} <= set(w["status"].tolist())


@pytest.mark.parametrize("wide", [False, True])
def test_decode_tables_cover_every_type_at_every_length(wide):
    pk = cc.decode_tables(wide)
    top = cc.MAX_PACKET_WIDE if wide else cc.MAX_PACKET
    assert {(p[0], len(p)) for p in pk if p} >= {(t, n) for t in list(range(8)) + [255] for n in range(1, top + 4)}
    assert sum(1 for p in pk if not p) == 9
    d = oracle.codec_decode_py(pk, wide=wide)
    assert set(d["status"].tolist()) == {0, 1, 2, 3}
    fb = set(bits(d["a"]).tolist()) | set(bits(d["b"]).tolist())
    quiet = {v | 0x00400000 if (v & 0x7FFFFFFF) > 0x7F800000 else v for v in cc.F32_PATTERNS}
    assert quiet <= fb and 0x80000000 in fb and len([v for v in fb if (v & 0x7FFFFFFF) > 0x7F800000]) >= 4
    body = [p for p in pk if len(p) == top + 3][1]   # neighbouring bytes differ: a field read one off shows
    assert all(x != y for x, y in zip(body[1:], body[2:]))


def test_decode_layouts_are_the_chunks_they_claim():
    lay = cc.decode_layouts()
    C = cc.DEC_CHUNK
    assert sorted(lay) == sorted(LAYOUT_NAMES)
    assert [len(lay["m%d" % m][1]) - 1 for m in (1, C - 1, C, C + 1, 2 * C + 1, 3 * C + 1)] == \
        [1, 1023, 1024, 1025, 2049, 3073]
    lds_bytes = C * 17 + 32
    for name, (buf, off, bad) in lay.items():
        d, inside = want_decode(buf, off, False)
        np.testing.assert_array_equal(np.flatnonzero(~inside), bad, err_msg=name)
        ends = off[np.r_[np.arange(0, len(off) - 1, C), len(off) - 1]]
        assert ends[0] == 0 and ends[-1] == len(buf) and (np.diff(ends) >= 0).all(), name
        if name != "oversized_packet":
            assert np.diff(ends).max() + 15 <= lds_bytes, name
        assert len(off) < 1000 or {0, 1} <= set(d["status"].tolist()), name
    buf, off, _ = lay["short_last_chunk"]
    assert 0 < off[-1] - off[C] < 16
    buf, off, _ = lay["oversized_packet"]
    assert np.diff(off).max() == 20_000 and off[-1] - off[C] > lds_bytes
    d, _ = want_decode(*lay["bad_offsets"][:2], False)
    assert (d["status"] == 4).sum() == 7


# ----------------------------------------------------------------------------- GPU

def dev_cols(cols):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64 if k in (3, 4) else torch.int64, device="cuda")
            for k, v in enumerate(cols)]


def encode_raw(cols, wide, out, cap, off, st):
    """swarm_codec_encode on these very device tensors (views keep their addresses) -> (rc, *total_bytes)."""
    from swarm_amd import _lib
    tot = ctypes.c_int64(-1)
    rc = _lib.lib().swarm_codec_encode(_lib.ctx(), cols[0].numel(), *[_lib.ptr(c) for c in cols], int(wide),
                                       _lib.ptr(out), cap, _lib.ptr(off), _lib.ptr(st), ctypes.byref(tot),
                                       _lib.stream())
    return rc, tot.value


def shifted(n, dtype, phase, fill=0):
    """A device tensor of n elements whose address is `phase` bytes past a 16-byte boundary."""
    import torch
    size = torch.empty(0, dtype=dtype).element_size()
    big = torch.full((n + 16 // size,), fill, dtype=dtype, device="cuda")
    v = big[phase // size:phase // size + n]
    assert big.data_ptr() % 16 == 0 and v.data_ptr() % 16 == phase
    return v


def check_encode_decode(name, cols, wide):
    """codec.encode, then codec.decode of its result, against the oracle -> list of differences."""
    from swarm_amd import codec
    w = want_encode(name, cols, wide)
    e = codec.encode(*cols, wide=wide, device="cuda")
    bad = [first_diff("status", e.status.cpu().numpy(), w["status"]),
           first_diff("offsets", e.offsets.cpu().numpy(), w["offsets"]),
           first_diff("bytes", e.buf.cpu().numpy(), w["buf"]),
           None if e.total_bytes == w["total"] else "total %d, want %d" % (e.total_bytes, w["total"])]
    want = oracle.codec_decode_py(w["packets"], wide=wide)
    d = codec.decode(e.buf, e.offsets, wide=wide, device="cuda")
    bad += [first_diff("decoded " + k, getattr(d, k).cpu().numpy(), want[k]) for k in DEC_KEYS]
    return [b for b in bad if b]


def check_tile_shape(name, cols, wide):
    """One case with `out` given and as a sizing call: status and offsets filled either way."""
    import torch
    from swarm_amd import _lib
    w = want_encode(name, cols, wide)
    m, dc, bad = len(cols[0]), dev_cols(cols), []
    for sizing in (False, True):
        off = torch.full((m + 1,), -7, dtype=torch.int64, device="cuda")
        st = torch.full((m,), -7, dtype=torch.int8, device="cuda")
        out = None if sizing else torch.full((w["total"] + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, tot = encode_raw(dc, wide, out, 0 if sizing else w["total"], off, st)
        tag = "sizing " if sizing else ""
        bad += [None if rc == _lib.OK else tag + "rc %d: %s" % (rc, _lib.last_error()),
                None if tot == w["total"] else tag + "total %d, want %d" % (tot, w["total"]),
                first_diff(tag + "status", st.cpu().numpy(), w["status"]),
                first_diff(tag + "offsets", off.cpu().numpy(), w["offsets"])]
        if not sizing:
            bad += [first_diff("bytes", out.cpu().numpy(), np.append(w["buf"], 0xA5).astype(np.uint8))]
    return [b for b in bad if b]


def check_placement(wide, phases=range(16)):
    """`out` = big[PAD + k:] inside a buffer of 0xA5: the oracle's bytes in [out, out + total), nothing else
    touched; caps that are too small report the needed size and leave [out + cap, ..) alone; the next call
    on the ctx is exact."""
    import torch
    from swarm_amd import _lib
    cols = cc.placement_batch()
    w = want_encode("placement", cols, wide)
    m, total, dc, bad = len(cols[0]), w["total"], dev_cols(cols), []
    off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(m, dtype=torch.int8, device="cuda")
    guard = np.full(2 * PAD + 15 + total, 0xA5, np.uint8)
    for k in phases:
        big = torch.full((len(guard),), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[PAD + k:]
        assert big.data_ptr() % 16 == 0 and out.data_ptr() % 16 == k
        for cap in (total - 1, int(w["offsets"][cc.TILE]), 0):   # too small: one byte, all but the first tile, all
            off.fill_(-7)
            rc, tot = encode_raw(dc, wide, out, cap, off, st)
            got = big.cpu().numpy()
            bad += [None if rc == _lib.ERR_RANGE and tot == total else "k=%d cap=%d: rc %d total %d" % (k, cap, rc, tot),
                    first_diff("k=%d cap=%d before out" % (k, cap), got[:PAD + k], guard[:PAD + k]),
                    first_diff("k=%d cap=%d from out + cap" % (k, cap), got[PAD + k + cap:], guard[PAD + k + cap:])]
            big.fill_(0xA5)
        off.fill_(-7)
        st.fill_(-7)
        rc, tot = encode_raw(dc, wide, out, total, off, st)   # cap == total
        want = guard.copy()
        want[PAD + k:PAD + k + total] = w["buf"]
        bad += [None if rc == _lib.OK and tot == total else "k=%d: rc %d total %d" % (k, rc, tot),
                first_diff("k=%d buffer" % k, big.cpu().numpy(), want),
                first_diff("k=%d status" % k, st.cpu().numpy(), w["status"]),
                first_diff("k=%d offsets" % k, off.cpu().numpy(), w["offsets"])]
    return [b for b in bad if b]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", ["field_edges", "float_edges"])
def test_gpu_field_and_float_edges(name, wide):
    assert check_encode_decode(name, encode_cases(wide)[name], wide) == []


@pytest.fixture(scope="module")
def tile_shapes():
    return cc.tile_shapes()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", TILE_NAMES)
def test_gpu_tile_shapes(tile_shapes, name, wide):
    assert check_tile_shape(name, tile_shapes[name], wide) == []


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_gpu_output_placement(wide):
    assert check_placement(wide) == []


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["status", "offsets", "type", "a", "winner"])
def test_gpu_single_misaligned_array(which):
    """One array alone off its alignment (status at an odd address, offsets or one input column at 8 mod 16)
    sends the call to the one-message-per-lane form: the aligned result."""
    import torch
    from swarm_amd import _lib
    cols = cc.placement_batch()
    w = want_encode("placement", cols, False)
    m, dc = len(cols[0]), dev_cols(cols)
    off = shifted(m + 1, torch.int64, 8 if which == "offsets" else 0, -7)
    st = shifted(m, torch.int8, 1 if which == "status" else 0, -7)
    if which in cc.COL:
        k = cc.COL[which]
        v = shifted(m, dc[k].dtype, 8)
        v.copy_(dc[k])
        dc[k] = v
    assert sum(t.data_ptr() % 16 != 0 for t in dc + [off, st]) == 1
    out = torch.full((w["total"] + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, tot = encode_raw(dc, False, out, w["total"], off, st)
    assert rc == _lib.OK and tot == w["total"]
    assert first_diff("status", st.cpu().numpy(), w["status"]) is None
    assert first_diff("offsets", off.cpu().numpy(), w["offsets"]) is None
    assert first_diff("bytes", out.cpu().numpy(), np.append(w["buf"], 0xA5).astype(np.uint8)) is None


def check_decode(buf, off, wide, phase, off_phase=0):
    """codec.decode with `buf` `phase` bytes and `offsets` `off_phase` bytes past a 16-byte boundary."""
    import torch
    from swarm_amd import codec
    want, _ = want_decode(buf, off, wide)
    db = shifted(len(buf), torch.uint8, phase)
    db.copy_(torch.as_tensor(np.asarray(buf), device="cuda"))
    do = shifted(len(off), torch.int64, off_phase)
    do.copy_(torch.as_tensor(off, device="cuda"))
    d = codec.decode(db, do, wide=wide, device="cuda")
    bad = [first_diff("phase %d+%d %s" % (phase, off_phase, k), getattr(d, k).cpu().numpy(), want[k]) for k in DEC_KEYS]
    return [b for b in bad if b]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_gpu_decode_tables(wide):
    buf, off = cc._layout(cc.decode_tables(wide))
    bad = [b for k in (0, 1, 7, 8, 15) for b in check_decode(buf, off, wide, k)]
    assert bad + check_decode(buf, off, wide, 0, 8) + check_decode(buf, off, wide, 7, 8) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUT_NAMES)
def test_gpu_decode_layouts(name):
    buf, off, _ = cc.decode_layouts()[name]
    bad = [b for k in (0, 1, 7, 8, 15) for b in check_decode(buf, off, False, k)]
    assert bad + check_decode(buf, off, False, 0, 8) + check_decode(buf, off, False, 15, 8) == []


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["SWARM_ENC_PASSES=3", "SWARM_ENC_PAIR=0", "SWARM_CODEC_WGS=1"])
def test_gpu_env_selected_forms(env):
    """The three-pass encode, the one-message-per-lane form and a single workgroup walking every decode chunk
    and place tile (with SWARM_ENC_PASSES=3 beside it) are chosen once per process: a child process runs the
    field edges, the tile shapes and the output placement (tests/codec_env_case.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    k, v = env.split("=")
    extra = {k: v, **({"SWARM_ENC_PASSES": "3"} if k == "SWARM_CODEC_WGS" else {})}
    p = subprocess.run([sys.executable, "-u", os.path.join(here, "codec_env_case.py")], env=dict(os.environ, **extra),
                       capture_output=True, text=True, timeout=300)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(lines[-1])
    assert res["ok"], (res["error"], [c for c in res["cases"] if not c["match"]])
    assert len(res["cases"]) == 2 * (2 + len(TILE_NAMES) + 1) + len(LAYOUT_NAMES)
