"""Deterministic edge cases of the wire codec (plain numpy, no HIP); tests/test_codec_edges.py says what each pins.

Encode cases are message columns in the argument order of ``oracle.codec_encode_py`` and
``codec.encode``: ``[type, sender, tick, a, b, task, winner]`` (int64, a / b float64).  Decode cases are
packets as ``bytes``, or a byte buffer with an offset array.  IDs stay below 256, so every message that
frames in the reference's layout frames with ``wide`` too.
"""
import numpy as np

HB, ACCLAIM, COORD, CLAIM, CONFLICT = 1, 2, 3, 4, 5
TYPES = (HB, ACCLAIM, COORD, CLAIM, CONFLICT)
MAX_PACKET, MAX_PACKET_WIDE = 14, 17
TILE = 2048        # messages per encode tile (8 waves x 256, two messages per lane)
DEC_CHUNK = 1024   # packets per decode chunk
FIELDS = ("sender", "tick", "task", "winner")
COL = dict(type=0, sender=1, tick=2, a=3, b=4, task=5, winner=6)
EDGE_INTS = (0, 255, 256, -1, 2**32 - 1, 2**32, 2**63 - 1, -2**63)
EDGE_TYPES = ((0, 6, 255, 256, 257, -1) + tuple(2**32 + k for k in range(1, 6)) +
              tuple(-2**32 + k for k in range(1, 6)) + (2**63 - 1, -2**63))
BASE = dict(sender=7, tick=1000, a=1.5, b=-2.25, task=77, winner=9)   # every field in range, no two alike


def _cols(rows):
    """[type, sender, tick, a, b, task, winner] columns of a list of dict(type=.., sender=.., ..)."""
    get = lambda k, dt: np.array([r[k] for r in rows], dt)  # noqa: E731
    return [get("type", np.int64), get("sender", np.int64), get("tick", np.int64), get("a", np.float64),
            get("b", np.float64), get("task", np.int64), get("winner", np.int64)]


def field_edges(wide):
    """Every type with each integer field, one at a time, at each of EDGE_INTS (the others as BASE), then every
    EDGE_TYPES value with BASE's fields.  `wide` does not change the messages (the same values are edges of
    both layouts); it is taken so that a caller names the layout it frames them for."""
    del wide
    rows = [dict(BASE, type=ty) for ty in TYPES]
    for ty in TYPES:
        for f in FIELDS:
            rows += [dict(BASE, type=ty, **{f: v}) for v in EDGE_INTS]
    rows += [dict(BASE, type=ty) for ty in EDGE_TYPES]
    return _cols(rows)


def _f64(bits):
    return float(np.array([bits], np.uint64).view(np.float64)[0])


F32_MIDPOINT = 2.0**128 - 2.0**103           # halfway from FLT_MAX to 2^128: rounds (to even) out of f32
FLT_MAX = 2.0**128 - 2.0**104
FLOAT_EDGES = (
    [0.0, -0.0, np.inf, -np.inf,
     _f64(0x7FF8000000000000), _f64(0xFFF8000000000000),                  # the quiet NaN of either sign
     _f64(0x7FF8000000000000 | (0x2AAAAA << 29)),                         # payload in the top 23 mantissa bits
     _f64(0xFFF0000000000000 | (0x2AAAAA << 29)),                         #   ... with the quiet bit clear
     _f64(0x7FF8000015555555), _f64(0xFFF0000015555555),                  # payload in the low 29 bits only
     _f64(0x7FF0000000000001)] +
    [s * v for s in (1.0, -1.0) for v in
     (2.0**-149, 2.0**-150, float(np.nextafter(2.0**-150, 1.0)), FLT_MAX, F32_MIDPOINT,
      float(np.nextafter(F32_MIDPOINT, 0.0)), float(np.nextafter(F32_MIDPOINT, np.inf)))])


def float_edges():
    """Heartbeats and claims with a / b at each of FLOAT_EDGES, one at a time (a claim does not frame b: no
    value of it is an error), and a heartbeat with both out of range."""
    rows = []
    for v in FLOAT_EDGES:
        rows += [dict(BASE, type=HB, a=v), dict(BASE, type=HB, b=v), dict(BASE, type=CLAIM, a=v),
                 dict(BASE, type=CLAIM, b=v)]
    rows.append(dict(BASE, type=HB, a=F32_MIDPOINT, b=-F32_MIDPOINT))
    return _cols(rows)


def mixed(m, seed, errors=0.03):
    """m seeded messages of all five types; a fraction `errors` of them with an unknown type, a field out of
    range or a float beyond f32 (statuses 3, 1, 2)."""
    rng = np.random.default_rng(seed)
    c = [rng.integers(1, 6, m), rng.integers(0, 256, m), rng.integers(0, 2**32, m), rng.normal(0, 1e3, m),
         rng.normal(0, 1e3, m), rng.integers(0, 2**32, m), rng.integers(0, 256, m)]
    kind = np.where(rng.uniform(size=m) < errors, rng.integers(1, 4, m), 0)
    c[0][kind == 3] = 2**32 + 3
    c[2][kind == 1] = 2**32
    c[3][kind == 2] = 3.5e38
    c[4][kind == 2] = -3.5e38
    c[5][kind == 2] = -1   # a claim checks its task before its utility: status 1 there, 2 on a heartbeat
    return c


def errors(m):
    """m messages that take no bytes: statuses 1, 2, 3 in turn."""
    c = _cols([dict(BASE, type=CONFLICT, task=-1), dict(BASE, type=HB, b=3.5e38), dict(BASE, type=2**32 + 1)])
    return [np.resize(v, m) for v in c]


def _cat(*parts):
    return [np.concatenate([p[k] for p in parts]) for k in range(7)]


def tile_shapes():
    """{name: columns}: message counts around the encode tile and tiles of extreme byte counts."""
    out = {}
    for m in (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 1, 65 * TILE + 1):
        out["m%d" % m] = mixed(m, 1000 + m)   # 65 tiles: a look-back longer than one 64-lane window
    out["error_tile_between"] = _cat(mixed(TILE, 1), errors(TILE), mixed(TILE, 2))
    coord = errors(TILE)                       # one 6-byte (wide: 9) COORDINATOR, else errors: the tile's bytes
    for k, v in zip(range(7), _cols([dict(BASE, type=COORD)])):   # end before its first 16-byte boundary
        coord[k][1301] = v[0]
    out["one_coordinator_tile"] = _cat(mixed(TILE, 3), coord, mixed(TILE, 4))
    out["first_tile_errors"] = _cat(errors(TILE), mixed(TILE + 5, 5))
    conflicts = [np.resize(v, TILE) for v in _cols([dict(BASE, type=CONFLICT, task=2**32 - 1, winner=255)])]
    conflicts[2] = np.arange(TILE, dtype=np.int64) * 2097143 + 1    # distinct ticks: a misplaced packet shows
    out["conflict_tile"] = _cat(mixed(TILE, 6), conflicts, mixed(TILE, 7))   # wide: 17 B each, a full LDS buffer
    return out


def placement_batch():
    """The three-tile batch of the output-placement tests (the third tile partly filled)."""
    return mixed(2 * TILE + 700, 42)


# ----------------------------------------------------------------------------- decode

F32_PATTERNS = (0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F812345, 0xFF800001, 0x7FFFFFFF,   # NaNs, quiet or not
                0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7F7FFFFF)   # -0.0, subnormals, inf


def decode_tables(wide):
    """Packets: every type byte 0..7 and 255 at every length 0..MAX_PACKET + 3, the bytes after the type from a
    running counter (no two neighbouring fields alike); then heartbeats and claims whose floats are
    F32_PATTERNS."""
    hdr, top = (9, MAX_PACKET_WIDE) if wide else (6, MAX_PACKET)
    pk, c = [], 0
    for ty in list(range(8)) + [255]:
        for n in range(top + 4):
            body = bytes((c + 1 + k) & 0xFF for k in range(max(n - 1, 0)))
            c += n
            pk.append((bytes([ty]) + body)[:n])
    head = lambda ty, q: bytes([ty]) + bytes((0x11 * (q + 1) + k) & 0xFF for k in range(hdr - 1))  # noqa: E731
    be = lambda v: int(v).to_bytes(4, "big")  # noqa: E731
    for q, bits in enumerate(F32_PATTERNS):
        other = F32_PATTERNS[(q + 5) % len(F32_PATTERNS)]
        pk.append(head(HB, q) + be(bits) + be(other))
        pk.append(head(CLAIM, q) + be(0xDEADBEEF - q) + be(bits))
    return pk


def _good_packets(m, seed):
    """m well-formed packets of the reference's layout, about one in sixteen cut short."""
    rng = np.random.default_rng(seed)
    ty = rng.integers(1, 6, m)
    n = 6 + np.array([0, 8, 1, 0, 8, 5])[ty]
    cut = rng.uniform(size=m) < 1 / 16
    n = np.where(cut, rng.integers(0, 14, m), n)
    raw = rng.integers(0, 256, (m, MAX_PACKET), dtype=np.uint8)
    raw[:, 0] = ty
    return [bytes(raw[i, :n[i]]) for i in range(m)]


def _layout(pk):
    off = np.concatenate([[0], np.cumsum([len(p) for p in pk])]).astype(np.int64)
    return np.frombuffer(b"".join(pk), np.uint8).copy(), off


def decode_layouts():
    """{name: (buf, offsets, bad)} for the 1 024-packet decode chunk (the reference's layout); `bad` lists the
    packets whose offsets must be refused (status 4).  Every other packet is buf[off[i]:off[i+1]]."""
    out = {}
    none = np.zeros(0, np.int64)
    for m in (1, DEC_CHUNK - 1, DEC_CHUNK, DEC_CHUNK + 1, 2 * DEC_CHUNK + 1, 3 * DEC_CHUNK + 1):
        out["m%d" % m] = _layout(_good_packets(m, 2000 + m)) + (none,)
    # a last chunk of two header-only packets: 12 bytes, no 16-byte word in it
    out["short_last_chunk"] = _layout(_good_packets(DEC_CHUNK, 11) + [bytes([COORD, 1, 2, 3, 4, 5])] * 2) + (none,)
    # one 20 000-byte packet (a heartbeat whose payload is not a position): its chunk does not fit the LDS buffer
    big = bytes([HB]) + bytes(k % 253 for k in range(19_999))
    pk = _good_packets(DEC_CHUNK + 300, 12)
    pk[DEC_CHUNK + 100] = big
    out["oversized_packet"] = _layout(pk) + (none,)
    # chunk endpoints (off[0], off[1024], off[2048], off[m]) in order; inside the second chunk single offsets that
    # run backwards, point before the chunk's first byte, past the buffer, below zero
    buf, off = _layout(_good_packets(2 * DEC_CHUNK + 50, 13))
    c = DEC_CHUNK
    off[c + 10] = off[c + 12]       # packet c+10 runs backwards (c+9 just grows)
    off[c + 100] = 5                # before the chunk's first byte: c+99 backwards, c+100 a long packet from byte 5
    off[c + 200] = len(buf) + 100   # past the buffer: c+199 ends outside, c+200 starts outside
    off[c + 300] = -3               # below zero
    off[c + 400] = off[c + 401] + 1  # one byte backwards
    bad = np.array([c + 10, c + 99, c + 199, c + 200, c + 299, c + 300, c + 400], np.int64)
    out["bad_offsets"] = (buf, off, bad)
    return out
