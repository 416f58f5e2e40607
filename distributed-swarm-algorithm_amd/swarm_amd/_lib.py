"""ctypes binding of libswarm.so (include/swarm.h).

The HIP path is the only compute path: if libswarm.so is missing or cannot load, every
batched call raises -- there is no CPU fallback.  torch is imported first so that the HIP
runtime torch ships (SONAME libamdhip64.so.7) is the one libswarm.so binds to: one runtime,
one set of device pointers and streams in the process.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must precede the CDLL: shares torch's HIP runtime)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libswarm.so")

OK, NOT_CONVERGED = 0, 1
ERR_ARG, ERR_HIP, ERR_OOM, ERR_RANGE, ERR_STALE = -1, -2, -3, -4, -5
FOLLOWER, ELECTION_WAIT, LEADER = 1, 2, 3
ELECT_DENSE, ELECT_FRONTIER, ELECT_TIMED, ELECT_TRUST_C16 = 0, 1, 0x100, 0x200
COMM_RCCL, COMM_SHM = 0, 1  # swarm_comm_create_kind transports
ALLOC_TRUST_INDEX, ALLOC_FRESH_CLAIMS = 1, 2  # swarm_allocate_indexed_ex flags
ALLOC_AUTO, ALLOC_BINNED, ALLOC_DENSE = 0, 1, 2

# every symbol include/swarm.h declares (tests/test_capi.py checks the two agree)
EXPORTS = ("swarm_last_error", "swarm_version", "swarm_ctx_create", "swarm_ctx_destroy",
           "swarm_elect", "swarm_elect_directed", "swarm_elect_i64", "swarm_elect_round", "swarm_allocate",
           "swarm_utility", "swarm_build_rgg", "swarm_cell_order", "swarm_frontier_begin",
           "swarm_frontier_step", "swarm_frontier_ghosts", "swarm_frontier_changes",
           "swarm_comm_available", "swarm_comm_unique_id", "swarm_comm_create", "swarm_comm_destroy",
           "swarm_elect_sharded", "swarm_auction", "swarm_physics_step", "swarm_codec_encode",
           "swarm_codec_decode", "swarm_protocol_run", "swarm_auction_begin",
           "swarm_auction_bid", "swarm_auction_resolve", "swarm_auction_sharded", "swarm_cell_index",
           "swarm_allocate_indexed", "swarm_graph_compact", "swarm_elect_compact",
           "swarm_elect_compact_i64", "swarm_frontier_begin_range", "swarm_frontier_set_compact",
           "swarm_comm_unique_id_kind", "swarm_comm_create_kind", "swarm_comm_kind", "swarm_allocate_indexed_ex",
           "swarm_protocol_run_ex", "swarm_elect_sharded_ex", "swarm_graph_compact_escaped",
           "swarm_frontier_set_compact_escaped", "swarm_physics_run_sensed", "swarm_update_loop",
           "swarm_update_loop_sensed", "swarm_update_loop_radio", "swarm_update_loop_tasks",
           "swarm_obstacle_field_create", "swarm_obstacle_field_obstacles", "swarm_obstacle_field_read",
           "swarm_obstacle_field_destroy", "swarm_update_loop_channel", "swarm_link_dropped",
           "swarm_obstacle_field_create_moving", "swarm_obstacle_field_set_velocities",
           "swarm_obstacle_field_refresh", "swarm_board_create", "swarm_board_info", "swarm_board_read",
           "swarm_board_destroy", "swarm_update_loop_board", "swarm_permute_rows", "swarm_graph_relabel",
           "swarm_resort_plan", "swarm_board_create_moving", "swarm_board_set_velocities", "swarm_board_positions",
           "swarm_board_refresh", "swarm_board_call_box", "swarm_update_loop_board_moving",
           "swarm_graph_pairs_count", "swarm_graph_pairs_fill", "swarm_elect_pairs", "swarm_board_census",
           "swarm_tasks_census", "swarm_board_set_lifetimes", "swarm_board_lifetimes", "swarm_board_place",
           "swarm_board_last_tick", "swarm_agent_life_create", "swarm_agent_life_set", "swarm_agent_life_events",
           "swarm_agent_life_destroy")
PLACE_KEEP_TABLES = 1  # swarm_board_place flags
BOARD_FITS, BOARD_STATUS, BOARD_TABLE = 0, 1, 2  # swarm_board_overflow.kind
BOARD_MAX_TASKS, BOARD_MAX_SLOTS = 1 << 24, 4096


class SwarmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libswarm error {code}: {msg}")
        self.code = code


class Fsm(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("state", "leader", "last_hb", "wait_start", "delay", "leader_pos",
                                               "has_leader_pos", "alive", "outbox")]


class Tasks(ctypes.Structure):
    """swarm_tasks: the board and every agent's task state (device pointers)."""
    _fields_ = [("T", ctypes.c_int32)] + \
               [(k, ctypes.c_void_p) for k in ("tpos", "treq", "caps", "status_lo", "status_hi", "claim_out",
                                               "conflict_out", "tab_winner", "tab_util")]


class Channel(ctypes.Structure):
    """swarm_channel: the lossy channel of swarm_update_loop_channel."""
    _fields_ = [("loss", ctypes.c_double), ("seed", ctypes.c_uint64)]


class BoardDesc(ctypes.Structure):
    """swarm_board_desc."""
    _fields_ = [("T", ctypes.c_int64), ("ncx", ctypes.c_int64), ("ncy", ctypes.c_int64), ("cell", ctypes.c_double),
                ("xmin", ctypes.c_double), ("ymin", ctypes.c_double), ("longest", ctypes.c_int64)]


class BoardState(ctypes.Structure):
    """swarm_board_state: every agent's sparse task state (device pointers)."""
    _fields_ = [("Ks", ctypes.c_int32), ("Kt", ctypes.c_int32)] + \
               [(k, ctypes.c_void_p) for k in ("caps", "status", "tab_task", "tab_winner", "tab_util", "claim_out",
                                               "conflict_out")]


CENSUS_FIELDS = ("tentative", "locked", "assigned", "tables", "holder_lo", "holder_hi", "winner_lo", "winner_hi",
                 "best_winner", "best_util")


class Census(ctypes.Structure):
    """swarm_census: the ten per-task arrays of a task census (device pointers)."""
    _fields_ = [(k, ctypes.c_void_p) for k in CENSUS_FIELDS]


class Rows(ctypes.Structure):
    """swarm_rows: one array of swarm_permute_rows (device pointers)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("row_bytes", ctypes.c_int64)]


class BoardOverflow(ctypes.Structure):
    """swarm_board_overflow."""
    _fields_ = [("kind", ctypes.c_int32), ("pad", ctypes.c_int32), ("agent", ctypes.c_int64)]


class ObstacleFieldInfo(ctypes.Structure):
    """swarm_obstacle_field_info."""
    _fields_ = [("m", ctypes.c_int64), ("live", ctypes.c_int64), ("ncx", ctypes.c_int64), ("ncy", ctypes.c_int64),
                ("cell", ctypes.c_double), ("xmin", ctypes.c_double), ("ymin", ctypes.c_double),
                ("pairs", ctypes.c_int64), ("longest", ctypes.c_int64)]


class AllocStats(ctypes.Structure):
    _fields_ = [("n_claims", ctypes.c_int64), ("n_conflicts", ctypes.c_int64),
                ("n_flagged", ctypes.c_int64), ("n_candidates", ctypes.c_int64),
                ("n_overflow", ctypes.c_int64), ("mode_used", ctypes.c_int64), ("n_resolved", ctypes.c_int64)]


class ElectStats(ctypes.Structure):
    _fields_ = [("rounds_launched", ctypes.c_int64), ("active_total", ctypes.c_int64),
                ("edges_total", ctypes.c_int64), ("changes_total", ctypes.c_int64),
                ("gather_ms", ctypes.c_double), ("apply_ms", ctypes.c_double),
                ("gather_launches", ctypes.c_int64), ("dense_rounds", ctypes.c_int64),
                ("bytes_total", ctypes.c_double), ("sparse_ms", ctypes.c_double),
                ("sparse_launches", ctypes.c_int64), ("sparse_bytes", ctypes.c_double),
                ("pair_launches", ctypes.c_int64)]


class AuctionStats(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int64), ("n_flagged", ctypes.c_int64),
                ("rounds_launched", ctypes.c_int64), ("tail_rounds", ctypes.c_int64),
                ("bids_total", ctypes.c_int64)]


class Grid(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("xmin", "ymin", "xmax", "ymax", "cell", "inv_cell")] + \
               [("ncx", ctypes.c_int64), ("ncy", ctypes.c_int64)]


class Shard(ctypes.Structure):
    """swarm_shard: one rank's rows and its peer list (the host arrays are kept alive by .keep)."""
    _fields_ = [("n_rows", ctypes.c_int64), ("n_all", ctypes.c_int64), ("row_ptr", ctypes.c_void_p),
                ("col", ctypes.c_void_p), ("init", ctypes.c_void_p), ("own_begin", ctypes.c_int64),
                ("halo_depth", ctypes.c_int32), ("n_peers", ctypes.c_int32), ("peers", ctypes.c_void_p),
                ("send_count", ctypes.c_void_p), ("send_rows", ctypes.c_void_p),
                ("ghost_count", ctypes.c_void_p), ("col16", ctypes.c_void_p), ("col16_escaped", ctypes.c_int32)]


def shard_desc(n_rows, n_all, row_ptr, col, init, own_begin, halo_depth, peers=(), send_count=(), send_rows=None,
               ghost_count=(), col16=None, col16_escaped=False) -> Shard:
    """A Shard over device tensors (row_ptr, col, init, send_rows, col16) and host peer lists."""
    import numpy as np
    pe = np.ascontiguousarray(peers, np.int32)
    sc = np.ascontiguousarray(send_count, np.int64)
    gc = np.ascontiguousarray(ghost_count, np.int64)
    z = ctypes.c_void_p(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else z  # noqa: E731
    dp = lambda t: ptr(t) if t is not None and t.numel() else z  # noqa: E731
    d = Shard(int(n_rows), int(n_all), dp(row_ptr), dp(col), dp(init), int(own_begin), int(halo_depth), len(pe),
              hp(pe), hp(sc), dp(send_rows), hp(gc), dp(col16), int(bool(col16_escaped)))
    d.keep = (pe, sc, gc)
    return d


_lib = None
_lock = threading.Lock()
_tls = threading.local()


def load(path: str = LIB_PATH):
    """Load libswarm.so (raises if it was not built -- run `make -C csrc`)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with "
                               f"`make -C distributed-swarm-algorithm_amd/csrc` (HIP path required)")
        L = ctypes.CDLL(path)
        P, i64, i32, d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
        L.swarm_last_error.restype = ctypes.c_char_p
        L.swarm_version.restype = ctypes.c_char_p
        L.swarm_ctx_create.argtypes = [ctypes.POINTER(P)]
        L.swarm_ctx_destroy.argtypes = [P]
        sig_elect = [P, i64, P, P, P, P, P, i32, i32, ctypes.POINTER(i32), P, P, P]
        L.swarm_elect.argtypes = sig_elect
        L.swarm_elect_i64.argtypes = sig_elect
        L.swarm_elect_directed.argtypes = [P, i64, P, P, P, P, P, P, P, i32, i32, ctypes.POINTER(i32), P, P, P]
        L.swarm_elect_round.argtypes = [P, i64, P, P, P, P, P, P]
        L.swarm_graph_compact.argtypes = [P, i64, P, P, P, P]
        L.swarm_elect_compact.argtypes = [P, i64, P, P, P, P, P, P, i32, i32, ctypes.POINTER(i32), P, P, P]
        L.swarm_elect_compact_i64.argtypes = [P, i64, P, P, P, P, P, P, i32, i32, ctypes.POINTER(i32), P, P, P]
        L.swarm_graph_pairs_count.argtypes = [P, i64, P, P, i32, P, P]
        L.swarm_graph_pairs_fill.argtypes = [P, i64, P, P, P, P, P]
        L.swarm_elect_pairs.argtypes = [P, i64, P, P, P, P, P, P, P, P, i32, i32, ctypes.POINTER(i32), P, P, P]
        L.swarm_allocate.argtypes = [P, i64, P, P, P, i64, P, P, d, d, d, i32, P, P, P, P, i64,
                                     P, P, P, P]
        L.swarm_utility.argtypes = [P, i64, P, P, P, P, d, P, P]
        L.swarm_cell_index.argtypes = [P, i64, P, d, ctypes.POINTER(Grid), P, i64, ctypes.POINTER(i64), P]
        L.swarm_allocate_indexed.argtypes = [P, i64, P, P, P, ctypes.POINTER(Grid), P, i64, P, P, d, d, d, P, P, P,
                                             P, i64, P, P, P, P]
        L.swarm_allocate_indexed_ex.argtypes = [P, i64, P, P, P, ctypes.POINTER(Grid), P, i64, P, P, d, d, d, i32, P, P, P,
                                             P, i64, P, P, P, P]
        L.swarm_build_rgg.argtypes = [P, i64, P, d, P, P, i64, ctypes.POINTER(i64), P]
        L.swarm_cell_order.argtypes = [P, i64, P, d, P, P]
        L.swarm_frontier_begin.argtypes = [P, i64, i64, P, P, P, P]
        L.swarm_frontier_begin_range.argtypes = [P, i64, i64, i64, P, P, P, P]
        L.swarm_frontier_set_compact.argtypes = [P, P]
        L.swarm_frontier_set_compact_escaped.argtypes = [P, P]
        L.swarm_graph_compact_escaped.argtypes = [P, i64, P, P, P, ctypes.POINTER(i64), P]
        L.swarm_frontier_step.argtypes = [P, i32, P, P, P, P, P]
        L.swarm_frontier_ghosts.argtypes = [P, i32, i64, i64, P, P, P, P, P, P]
        L.swarm_frontier_changes.argtypes = [P, i32, i32, P, P]
        L.swarm_comm_available.argtypes = []
        L.swarm_comm_unique_id.argtypes = [P]
        L.swarm_comm_create.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.c_int, P]
        L.swarm_comm_unique_id_kind.argtypes = [ctypes.c_int, P]
        L.swarm_comm_create_kind.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
        L.swarm_comm_kind.argtypes = [P]
        L.swarm_comm_destroy.argtypes = [P]
        L.swarm_elect_sharded.argtypes = [P, P, ctypes.POINTER(Shard), P, P, i32, ctypes.POINTER(i32), P, P]
        L.swarm_elect_sharded_ex.argtypes = [P, P, ctypes.POINTER(Shard), P, P, i32, ctypes.POINTER(i32), P, P, P, P]
        L.swarm_physics_step.argtypes = [P, i64, P, P, P, P, P, P, P, P, i64, P, P, P, d, d, ctypes.POINTER(i64), P]
        L.swarm_physics_run_sensed.argtypes = [P, i64, P, P, P, P, P, P, P, i64, P, d, i32, d, d, ctypes.POINTER(i32),
                                               ctypes.POINTER(i64), P]
        L.swarm_codec_encode.argtypes = [P, i64, P, P, P, P, P, P, P, i32, P, i64, P, P, ctypes.POINTER(i64), P]
        L.swarm_codec_decode.argtypes = [P, i64, P, i64, P, i32, P, P, P, P, P, P, P, P, P, P]
        L.swarm_protocol_run.argtypes = [P, i64, P, P, P, P, P, P, P, ctypes.POINTER(Fsm), i64, i32, d, d, d,
                                         ctypes.c_uint64, P, i32, P, P]
        L.swarm_protocol_run_ex.argtypes = [P, i64, P, P, P, P, P, P, P, ctypes.POINTER(Fsm), i64, i32, d, d, d,
                                            ctypes.c_uint64, P, i32, d, P, P, P]
        L.swarm_update_loop.argtypes = [P, i64, P, P, P, P, P, P, P, P, ctypes.POINTER(Fsm), i64, i32, d, d, d,
                                        ctypes.c_uint64, P, i32, d, P, P, P, i64, P, P, P, d, P, i32, P,
                                        ctypes.POINTER(i64), P]
        L.swarm_update_loop_sensed.argtypes = [P, i64, P, P, P, P, P, P, P, P, ctypes.POINTER(Fsm), i64, i32, d, d, d,
                                               ctypes.c_uint64, P, i32, d, P, P, P, i64, P, d, d, P, i32, P,
                                               ctypes.POINTER(i64), ctypes.POINTER(i64), P]
        L.swarm_update_loop_radio.argtypes = [P, i64, P, P, P, P, ctypes.POINTER(Fsm), i64, i32, d, d, d,
                                              ctypes.c_uint64, P, i32, P, P, P, i64, P, d, d, d, P, i32, P,
                                              ctypes.POINTER(i64), ctypes.POINTER(i64), P]
        L.swarm_update_loop_tasks.argtypes = L.swarm_update_loop_radio.argtypes[:-1] + [
            ctypes.POINTER(Tasks), P, ctypes.POINTER(i64), P]
        L.swarm_update_loop_channel.argtypes = L.swarm_update_loop_tasks.argtypes + [ctypes.POINTER(Channel), P]
        L.swarm_link_dropped.argtypes = [ctypes.c_uint64, i64, i32, i32, d]
        L.swarm_auction_begin.argtypes = [P, i64, P, P, P, i64, P, P, d, d, ctypes.c_float, P, P, P, P, P]
        L.swarm_auction_bid.argtypes = [P, i64, i32, i32, P, P, P, P]
        L.swarm_auction_resolve.argtypes = [P, i64, i32, P, P, P, P, P, P]
        L.swarm_auction_sharded.argtypes = [P, P, i64, P, P, P, i64, P, P, d, d, ctypes.c_float, i32, P, P, P,
                                            ctypes.POINTER(i32), P, P, P]
        L.swarm_auction.argtypes = [P, i64, P, P, P, i64, P, P, d, d, ctypes.c_float, i32, P, P, P,
                                    ctypes.POINTER(i32), P, P, P]
        L.swarm_obstacle_field_create.argtypes = [P, i64, P, ctypes.POINTER(P), ctypes.POINTER(ObstacleFieldInfo), P]
        L.swarm_obstacle_field_obstacles.argtypes = [P, ctypes.POINTER(P)]
        L.swarm_obstacle_field_read.argtypes = [P, P, P]
        L.swarm_obstacle_field_destroy.argtypes = [P, P]
        L.swarm_obstacle_field_create_moving.argtypes = [P, i64, P, P, ctypes.POINTER(P),
                                                         ctypes.POINTER(ObstacleFieldInfo), P]
        L.swarm_obstacle_field_set_velocities.argtypes = [P, P, P, P]
        L.swarm_obstacle_field_refresh.argtypes = [P, P, ctypes.POINTER(ObstacleFieldInfo), P]
        L.swarm_board_create.argtypes = [P, i64, P, P, ctypes.POINTER(P), ctypes.POINTER(BoardDesc), P]
        L.swarm_board_info.argtypes = [P, ctypes.POINTER(BoardDesc)]
        L.swarm_board_read.argtypes = [P, P, P]
        L.swarm_board_destroy.argtypes = [P, P]
        L.swarm_update_loop_board.argtypes = L.swarm_update_loop_radio.argtypes[:-1] + [
            P, ctypes.POINTER(BoardState), P, ctypes.POINTER(i64), P, ctypes.POINTER(Channel), P,
            ctypes.POINTER(BoardOverflow)]
        L.swarm_board_create_moving.argtypes = [P, i64, P, P, P, ctypes.POINTER(P), ctypes.POINTER(BoardDesc), P]
        L.swarm_board_set_velocities.argtypes = [P, P, P, P]
        L.swarm_board_positions.argtypes = [P, ctypes.POINTER(P), ctypes.POINTER(P)]
        L.swarm_board_set_lifetimes.argtypes = [P, P, P, P, P]
        L.swarm_board_lifetimes.argtypes = [P, ctypes.POINTER(P), ctypes.POINTER(P)]
        L.swarm_board_place.argtypes = [P, P, i64, ctypes.POINTER(BoardState), i64, P, P, P, P, P, P, ctypes.c_uint32,
                                        ctypes.POINTER(i64), P]
        L.swarm_board_last_tick.argtypes = [P, ctypes.POINTER(i64)]
        L.swarm_board_refresh.argtypes = [P, P, ctypes.POINTER(BoardDesc), P]
        L.swarm_board_call_box.argtypes = [P, P, d, i32, P, P]
        L.swarm_update_loop_board_moving.argtypes = L.swarm_update_loop_board.argtypes
        L.swarm_board_census.argtypes = [P, i64, P, P, ctypes.POINTER(BoardState), P, ctypes.POINTER(Census), P, i64,
                                         ctypes.POINTER(i64), P]
        L.swarm_tasks_census.argtypes = [P, i64, P, i32, P, P, P, P, P, ctypes.POINTER(Census), P, i64,
                                         ctypes.POINTER(i64), P]
        L.swarm_permute_rows.argtypes = [P, i64, P, i32, ctypes.POINTER(Rows), P]
        L.swarm_graph_relabel.argtypes = [P, i64, P, P, P, P, P, P]
        L.swarm_resort_plan.argtypes = [P, i64, P, P, d, P, P, ctypes.POINTER(i64), P]
        L.swarm_agent_life_create.argtypes = [P, i64, P, P, P, P, ctypes.POINTER(P)]
        L.swarm_agent_life_set.argtypes = [P, P, i64, P, P, i64, P]
        L.swarm_agent_life_events.argtypes = [P, P, i64, i32, P]
        L.swarm_agent_life_destroy.argtypes = [P, P]
        for name in EXPORTS:
            if name not in ("swarm_last_error", "swarm_version"):
                getattr(L, name).restype = ctypes.c_int
        _lib = L
        return L


def lib():
    return _lib if _lib is not None else load()


def last_error() -> str:
    """This thread's libswarm error text (swarm_last_error)."""
    return lib().swarm_last_error().decode(errors="replace")


def check(rc: int):
    if rc < 0:
        raise SwarmError(rc, last_error())
    return rc


class Ctx:
    """An owned swarm_ctx (scratch + frontier-stepper state) on the device current at creation.
    libswarm refuses a ctx on any other device (SWARM_ERR_ARG)."""

    def __init__(self):
        self.handle = ctypes.c_void_p()
        check(lib().swarm_ctx_create(ctypes.byref(self.handle)))
        self.device = torch.cuda.current_device() if torch.cuda.is_available() else -1

    @property
    def _as_parameter_(self):  # ctypes passes the raw handle
        return self.handle

    def __del__(self):
        h, L = getattr(self, "handle", None), _lib
        if h is not None and h.value and L is not None:
            L.swarm_ctx_destroy(h)
            self.handle = ctypes.c_void_p()


def ctx():
    """This thread's scratch context for the current device (one per (thread, device): scratch
    buffers belong to the device they were allocated on)."""
    per = getattr(_tls, "ctx", None)
    if per is None:
        per = _tls.ctx = {}
    dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
    c = per.get(dev)
    if c is None:
        c = per[dev] = Ctx()
    return c


def version() -> str:
    return lib().swarm_version().decode()


CSRC = os.path.join(os.path.dirname(HERE), "csrc")
INCLUDE_H = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "swarm.h")


def source_hash() -> str:
    """sha256 prefix of this tree's library sources, as csrc/Makefile computes it for the build:
    *.hip and *.h of csrc/ sorted by name, then csrc/Makefile, then include/swarm.h."""
    import hashlib
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    h = hashlib.sha256()
    for p in [os.path.join(CSRC, f) for f in names] + [os.path.join(CSRC, "Makefile"), INCLUDE_H]:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def built_hash() -> str:
    """The source hash libswarm.so was built from (parsed from swarm_version())."""
    v = version()
    return v.split("src=", 1)[1].strip() if "src=" in v else ""


def provenance() -> dict:
    """Which build is loaded, and whether it matches this tree's sources."""
    b, t = built_hash(), source_hash()
    return {"libswarm": LIB_PATH, "version": version(), "src_hash_built": b, "src_hash_tree": t,
            "matches_tree": b == t}


def ptr(t, dtype=None, numel=None, name="tensor"):
    """Device pointer of a contiguous CUDA tensor (validated), or None."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA tensor")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if numel is not None and t.numel() < numel:
        raise ValueError(f"{name}: needs >= {numel} elements, has {t.numel()}")
    return ctypes.c_void_p(t.data_ptr())


def copy_to_host(out, dev_ptr):
    """out (a contiguous numpy array) <- the device memory at dev_ptr, through the HIP runtime libswarm.so is
    linked against (a blocking copy; the caller has waited for the stream that wrote the memory)."""
    f = lib().hipMemcpy
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
    rc = f(out.ctypes.data_as(ctypes.c_void_p), dev_ptr, out.nbytes, 2)  # hipMemcpyDeviceToHost
    if rc != 0:
        raise SwarmError(ERR_HIP, f"hipMemcpy device -> host failed ({rc})")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
