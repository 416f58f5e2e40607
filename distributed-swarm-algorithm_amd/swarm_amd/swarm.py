"""Batched, HBM-resident swarm: the GPU face of the reference's per-round handlers.

One ``Swarm`` holds every agent as structure-of-arrays in device memory (SURVEY §2 "SoA swarm
state"): ``ids`` int32, ``pos`` float64 (x, y) pairs, ``caps`` uint32 bitmask, the neighbour
CSR (``row_ptr`` int32, ``col`` int32) and the election outputs ``leader`` int32 / ``state``
uint8.  Agents are stored in spatial (grid-cell) order by default, so a neighbour gather and a
task's candidate scan touch nearby memory; ``perm`` maps storage index -> input index.

  elect()     all rounds of contract E2 to convergence  -> swarm_elect (libswarm.so)
              (SwarmAgent._handle_election_acclaim / _handle_heartbeat, agent.py:243-275)
  allocate()  one claim/resolve/notify round             -> swarm_allocate
              (SwarmAgent._process_tasks / _handle_task_claim / _handle_task_conflict /
               _calculate_utility, agent.py:292-347)

Every compute call goes through the HIP kernels; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib

# swarm_elect_compact's edge cap with 16-bit columns (elect.hip check_graph: 32-bit byte offsets into
# the int16 columns, less a margin for the clamped offsets past a row's end)
_C16_EDGE_CAP = (1 << 31) - (1 << 20)


def _c16_rounds() -> bool:
    """Every round of swarm_elect_compact reads the 16-bit columns (the A/B knobs of elect.hip's
    tuning(): SWARM_C16 and SWARM_DENSE_FLAT, both on by default)."""
    return os.environ.get("SWARM_C16", "1") != "0" and os.environ.get("SWARM_DENSE_FLAT", "1") != "0"


CAP_VOCAB_DEFAULT = ("extinguisher", "sonar", "camera", "gripper")
STATUS_NAMES = ("OPEN", "TENTATIVE", "LOCKED", "ASSIGNED")
# Capability bit reserved for "a required capability no agent holds" (a task dict naming a
# capability outside the vocabulary: agent.py:344 gives every agent has_cap = 0 for it).  The
# bridge never sets it on an agent, so vocabularies hold at most 31 names.
CAP_UNHELD_BIT = 31


def _dev(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("swarm_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _to(a, dtype, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:  # torch refuses read-only buffers (np.frombuffer, np.load views)
        a = a.copy()
    return torch.as_tensor(a, dtype=dtype, device=device)


# Pair rounds (elect.hip, "pair rounds"): the frontier election's tail runs two rounds per launch
# through a two-hop index of the graph.  Swarms of at least SWARM_PAIR_MIN_AGENTS agents build the index on their
# first frontier election of a graph version and use it by default (Swarm.elect(pairs=...) overrides).
# The default is the A/B of tools/elect_ab.py at 1M and 10M agents (DESIGN_LOG.md): PAIR_MIN_AGENTS_DEFAULT.
PAIR_MIN_AGENTS_DEFAULT = 1_000_000
# rows longer than this refuse the index (hub rows: a riser's row is walked by 4 or 8 lanes); a degree-16 radius
# graph's longest two-hop row is ~90
PAIR_ROW_CAP = 512


def _pair_min_agents() -> int:
    return int(os.environ.get("SWARM_PAIR_MIN_AGENTS", PAIR_MIN_AGENTS_DEFAULT))


# SWARM_TRUST_C16=0 (A/B aid): every election re-checks the 16-bit columns on the device
_TRUST_C16 = _lib.ELECT_TRUST_C16 if os.environ.get("SWARM_TRUST_C16", "1") != "0" else 0


@dataclass
class ElectResult:
    rounds_exec: int
    changes: np.ndarray                 # per-round change counts, rounds 1..rounds_exec
    leader: torch.Tensor                # int32 [n], storage order
    state: torch.Tensor                 # uint8 [n], storage order (1 FOLLOWER, 3 LEADER)
    converged: bool = True
    rounds_launched: int = 0
    active_total: int = 0               # agents gathered (dense: all, sparse: marked -- stamped by a riser under
                                        # elect.hip's SWARM_MARK_PRUNE rule), summed over rounds
    edges_total: int = 0                # CSR edges visited, summed over rounds
    dense_rounds: int = 0               # rounds run as a full dense sweep
    bytes_total: float = 0.0            # algorithmic HBM bytes of rounds 1..rounds_exec


@dataclass
class AuctionResult:
    owner: torch.Tensor                 # int32 [t] storage index of the task's agent (-1 = none)
    price: torch.Tensor                 # float32 [t] final prices
    assigned: torch.Tensor              # int32 [n] task index per agent (storage order, -1 = none)
    rounds_exec: int                    # rounds that had bidders
    bidders: np.ndarray                 # per-round bidder counts, rounds 1..rounds_exec
    converged: bool = True
    stats: dict = field(default_factory=dict)


@dataclass
class AllocResult:
    winner: torch.Tensor                # int32 [t] (-1 = unclaimed)
    util: torch.Tensor                  # float64 [t] winning claim value (f32-valued)
    won: torch.Tensor                   # int32 [n] tasks won per agent (storage order)
    nclaim: torch.Tensor                # int64 [t] TASK_CLAIMs per task
    nmsg: torch.Tensor                  # int64 [t] TASK_CONFLICTs per task
    stats: dict = field(default_factory=dict)


def _fast_ptr(t):
    """Device pointer of a tensor this module made or owns (contiguous, on the right device): no
    validation (allocate's per-call host cost; user tensors go through _lib.ptr)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _tensor_rec(t):
    """What a cache derived from tensor `t` records of it: the tensor OBJECT, held weakly (the cache must not
    keep a replaced graph's memory alive), and its version counter.  Never its address: the caching allocator
    hands a freed block to the next tensor of that size, and a new tensor starts at version 0 again."""
    return (weakref.ref(t), t._version)


def _same_tensor(rec, t) -> bool:
    """`t` is the very tensor object, at the same version, that `rec` (_tensor_rec) recorded.  False for
    another object over the same memory (a .data alias, a new tensor at a recycled address), after an
    in-place write, and once the recorded tensor is gone (a dead reference matches nothing)."""
    return rec is not None and t is not None and rec[0]() is t and rec[1] == t._version


def take_rows(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """t[idx] for a 2-D tensor, gathered one column at a time.  On this PyTorch-ROCm build the
    row gathers of an (N, 2) float64 tensor (t[idx], index_select, gather) return wrong rows
    above 2^26 rows, while 1-D gathers are right (checked on MI355X at 68M and 140M rows); the
    wrong positions piled 67M agents into one grid cell, and the graph build then never ended."""
    if t.dim() != 2:
        return t[idx].contiguous()
    return torch.stack([t[:, j].contiguous()[idx] for j in range(t.shape[1])], 1).contiguous()


def _destroy_field(ctx, handle):
    """ObstacleField's finalizer: `ctx` is held so that the ctx outlives its field (a ctx on another device
    than the current one refuses the call: its own device is made current for it)."""
    L = _lib._lib
    if L is not None and handle.value and ctx.handle.value:
        with torch.cuda.device(ctx.device):
            L.swarm_obstacle_field_destroy(ctx.handle, handle)
    handle.value = None


def _board_velocities(v, T):
    """set_task_board / set_board_velocities: a (T, 2) float64 array of finite velocities."""
    vel = np.ascontiguousarray(np.asarray(v, np.float64))
    if vel.shape != (T, 2):
        raise ValueError(f"velocities: expected shape ({T}, 2), got {tuple(vel.shape)}")
    if not np.isfinite(vel).all():
        raise ValueError("velocities must be finite")
    return vel


LIFE_FOREVER = np.iinfo(np.int64).max


def _board_lifetimes(open_tick, close_tick, T):
    """set_task_board / set_board_lifetimes: the (T,) int64 windows of open_tick / close_tick, each (T,) ints or a
    scalar; None for open_tick is tick 0, for close_tick never (contract U1-A).  (None, None): no lifetimes."""
    if open_tick is None and close_tick is None:
        return None
    out = []
    for name, v, default in (("open_tick", open_tick, 0), ("close_tick", close_tick, LIFE_FOREVER)):
        a = np.asarray(default if v is None else v)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be integer ticks, got dtype {a.dtype}")
        if a.dtype.kind == "u" and a.size and int(a.max()) > LIFE_FOREVER:
            raise ValueError(f"{name} must fit a signed 64-bit tick")
        if a.ndim == 0:
            a = np.full(T, int(a), np.int64)
        if a.shape != (T,):
            raise ValueError(f"{name}: expected {T} ticks or a scalar, got shape {tuple(a.shape)}")
        out.append(np.ascontiguousarray(a.astype(np.int64)))
    lo, hi = out
    if T and (int(lo.min()) < 0 or int(hi.min()) < 0):
        raise ValueError("open_tick and close_tick must not be negative")
    if (lo > hi).any():
        raise ValueError(f"task {int(np.argmax(lo > hi))} opens after it closes")
    return lo, hi


AGENT_BOOT_MAX = 1 << 31


def _agent_lifetimes(boot_tick, death_tick, n):
    """set_agent_lifetimes: the (n,) int64 windows of boot_tick / death_tick, each (n,) ints or a scalar; None for
    boot_tick is tick 0, for death_tick never (contract U1-J).  (None, None): no lifetimes."""
    if boot_tick is None and death_tick is None:
        return None
    out = []
    for name, v, default in (("boot_tick", boot_tick, 0), ("death_tick", death_tick, LIFE_FOREVER)):
        a = np.asarray(default if v is None else v)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be integer ticks, got dtype {a.dtype}")
        if a.dtype.kind == "u" and a.size and int(a.max()) > LIFE_FOREVER:
            raise ValueError(f"{name} must fit a signed 64-bit tick")
        if a.ndim == 0:
            a = np.full(n, int(a), np.int64)
        if a.shape != (n,):
            raise ValueError(f"{name}: expected {n} ticks or a scalar, got shape {tuple(a.shape)}")
        out.append(np.ascontiguousarray(a.astype(np.int64)))
    boot, death = out
    if n and (int(boot.min()) < 0 or int(boot.max()) >= AGENT_BOOT_MAX):
        raise ValueError("boot_tick must be in [0, 2^31)")
    if n and int(death.min()) < 0:
        raise ValueError("death_tick must not be negative")
    return boot, death


def _destroy_agent_life(ctx, handle):
    """The finalizer of a swarm's agent lifetimes (set_agent_lifetimes), as _destroy_field."""
    L = _lib._lib
    if L is not None and handle.value and ctx.handle.value:
        with torch.cuda.device(ctx.device):
            L.swarm_agent_life_destroy(ctx.handle, handle)
    handle.value = None


def _destroy_board(ctx, handle):
    """A task board's finalizer (set_task_board), as _destroy_field."""
    L = _lib._lib
    if L is not None and handle.value and ctx.handle.value:
        with torch.cuda.device(ctx.device):
            L.swarm_board_destroy(ctx.handle, handle)
    handle.value = None


BOARD_OVERFLOW_KINDS = {_lib.BOARD_STATUS: "status", _lib.BOARD_TABLE: "table"}


class ObstacleField:
    """An obstacle field (contract O1, swarm_obstacle_field): a list of m obstacles (x, y, r) with, per cell
    of a grid over them, the obstacles that can act on an agent there.  Made by Swarm.obstacle_field();
    read-only.  Pass it wherever an `obstacles=` list goes: the sensed calls (physics_step with sense_radius,
    update_loop_sensed / _radio / _tasks) then visit only the obstacles in an agent's reach, the fixed-graph
    calls read its list -- every result bit-identical to the same call with the list.  The field belongs to
    the calling thread's ctx of its device; from another thread the calls read it as the flat list.

    With `velocities` (m x 2; contract O2) the field moves: every tick of a sensed call reads the list
    as it stands, then every obstacle advances by fl(v * dt).  The field owns the current list (positions()),
    `obstacles` stays the creation list.  The fixed-graph calls (physics_step without sense_radius, update_loop)
    and a ctx or device other than the field's own raise: they would read the list as a frozen one."""

    def __init__(self, obstacles, device, velocities=None):
        import weakref
        dev = device if isinstance(device, torch.device) else _dev(device)
        # (always a copy: later writes to the caller's tensor must not reach the field)
        src = torch.tensor(np.asarray(obstacles.detach().cpu() if isinstance(obstacles, torch.Tensor) else obstacles,
                                      dtype=np.float64).reshape(-1, 3))
        self.obstacles = src.numpy().copy()
        self.obstacles.flags.writeable = False
        self.m, self.device = int(src.shape[0]), dev
        self.moving = velocities is not None
        info, self._handle = _lib.ObstacleFieldInfo(), ctypes.c_void_p()
        with torch.cuda.device(dev):
            d_obs = src.to(dev)
            self._ctx = _lib.ctx()
            if self.moving:
                d_vel = self._velocities(velocities)
                _lib.check(_lib.lib().swarm_obstacle_field_create_moving(
                    self._ctx, self.m, _lib.ptr(d_obs) if self.m else None, _lib.ptr(d_vel) if self.m else None,
                    ctypes.byref(self._handle), ctypes.byref(info), _lib.stream()))
            else:
                _lib.check(_lib.lib().swarm_obstacle_field_create(
                    self._ctx, self.m, _lib.ptr(d_obs) if self.m else None, ctypes.byref(self._handle),
                    ctypes.byref(info), _lib.stream()))
        self.info = {k: getattr(info, k) for k, _ in _lib.ObstacleFieldInfo._fields_}
        self._ptr = ctypes.c_void_p()
        _lib.check(_lib.lib().swarm_obstacle_field_obstacles(self._handle, ctypes.byref(self._ptr)))
        self._finalizer = weakref.finalize(self, _destroy_field, self._ctx, self._handle)

    @property
    def closed(self) -> bool:
        return not self._finalizer.alive

    def _check_open(self):
        if self.closed:
            raise ValueError("the obstacle field is closed")

    def read(self):
        """(cell_off uint32 [ncx * ncy + 1], idx int32 [pairs]): cell c = cy * ncx + cx lists the obstacles
        idx[cell_off[c]:cell_off[c + 1]], ascending."""
        self._check_open()
        off = np.zeros(self.info["ncx"] * self.info["ncy"] + 1, np.uint32)
        idx = np.zeros(self.info["pairs"], np.int32)
        _lib.check(_lib.lib().swarm_obstacle_field_read(self._handle, off.ctypes.data_as(ctypes.c_void_p),
                                                        idx.ctypes.data_as(ctypes.c_void_p)))
        return off, idx

    def _velocities(self, v):
        """The (m, 2) float64 device tensor of a velocities argument; ValueError for another shape."""
        a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
        if a.shape != (self.m, 2):
            raise ValueError(f"velocities must have shape ({self.m}, 2), got {a.shape}")
        return torch.tensor(a).to(self.device).contiguous()

    def _own_ctx(self):
        """The field's ctx, which must be the calling thread's ctx of the field's device."""
        self._check_open()
        with torch.cuda.device(self.device):
            if _lib.ctx() is not self._ctx:
                raise ValueError("a moving obstacle field can only be used from the thread (ctx) that made it")
        return self._ctx

    def positions(self) -> np.ndarray:
        """The current (m, 3) list: the creation list of a static field, where the ticks so far have carried
        the obstacles of a moving one."""
        self._check_open()
        if not self.moving or self.m == 0:
            return self.obstacles.copy()
        out = np.empty((self.m, 3), np.float64)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.copy_to_host(out, self._ptr)
        return out

    def set_velocities(self, velocities):
        """New velocities (m x 2) from the next tick on (swarm_obstacle_field_set_velocities)."""
        self._check_open()
        if not self.moving:
            raise ValueError("the obstacle field does not move: make it with velocities")
        d_vel = self._velocities(velocities)
        ctx = self._own_ctx()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().swarm_obstacle_field_set_velocities(
                ctx, self._handle, _lib.ptr(d_vel) if self.m else None, _lib.stream()))

    def refresh(self):
        """The cell lists of the current list, rebuilt by the device builder on the grid a static field of that
        list would get (swarm_obstacle_field_refresh); updates `info`, and read() returns those lists."""
        self._check_open()
        info = _lib.ObstacleFieldInfo()
        ctx = self._own_ctx() if self.moving else self._ctx
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().swarm_obstacle_field_refresh(ctx, self._handle, ctypes.byref(info), _lib.stream()))
        self.info = {k: getattr(info, k) for k, _ in _lib.ObstacleFieldInfo._fields_}
        return self.info

    def close(self):
        """Frees the field (waits for the device first).  Using it afterwards raises ValueError."""
        if not self.closed:
            with torch.cuda.device(self.device):
                self._finalizer()

    def _args(self, dev):
        """(m, device pointer of the field's own list) for a call on device `dev`."""
        self._check_open()
        if dev != self.device:
            raise ValueError(f"the obstacle field lives on {self.device}, the swarm on {dev}")
        if self.moving:
            self._own_ctx()
        return self.m, self._ptr


def _channel(loss, loss_seed):
    """The radio loops' loss keywords -> (loss, seed) for swarm_update_loop_channel, or None for the ideal
    channel (the loss-free entry points, exactly as without the keywords)."""
    loss = float(loss)
    if not 0.0 <= loss <= 1.0:  # (NaN fails both comparisons)
        raise ValueError(f"loss must be in [0, 1], got {loss}")
    return (loss, int(loss_seed) & 0xFFFFFFFFFFFFFFFF) if loss > 0.0 else None


def _no_moving_field(obstacles, what):
    """The fixed-graph calls refuse a moving field: they would read its list as a frozen one (contract O2)."""
    if isinstance(obstacles, ObstacleField) and obstacles.moving:
        raise ValueError(f"{what} cannot take a moving obstacle field: use a sensed call")


def _obstacle_args(obstacles, dev):
    """(m, pointer or None, keep-alive) of an `obstacles=` argument: a list or an ObstacleField."""
    if isinstance(obstacles, ObstacleField):
        return (*obstacles._args(dev), obstacles)
    obs = torch.zeros((0, 3), dtype=torch.float64, device=dev) if obstacles is None else \
        _to(obstacles, torch.float64, dev).reshape(-1, 3).contiguous()
    return obs.shape[0], (_lib.ptr(obs) if obs.numel() else None), obs


class Swarm:
    """Structure-of-arrays swarm resident on one GPU."""

    def __init__(self, ids, x, y, caps=None, *, layout: str = "spatial", cell: float = 1.0,
                 device=None):
        dev = _dev(device)
        _lib.lib()
        self.device = dev
        ids_t = _to(ids, torch.int32, dev)
        n = ids_t.numel()
        pos = torch.stack([_to(x, torch.float64, dev), _to(y, torch.float64, dev)], dim=1).contiguous()
        if caps is None:
            caps = np.zeros(n, np.uint32)
        if not isinstance(caps, torch.Tensor):  # uint32 bitmask, carried bit-for-bit as int32
            caps = np.ascontiguousarray(caps, dtype=np.uint32).view(np.int32)
        caps_t = _to(caps, torch.int32, dev)
        self.n = n
        if layout == "spatial" and n > 1:
            perm = torch.empty(n, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().swarm_cell_order(_lib.ctx(), n, _lib.ptr(pos, torch.float64),
                                                       float(cell), _lib.ptr(perm), _lib.stream()))
            p = perm.long()
            ids_t, pos, caps_t = ids_t[p].contiguous(), take_rows(pos, p), caps_t[p].contiguous()
            self.perm = perm
        elif layout in ("spatial", "input"):
            self.perm = torch.arange(n, dtype=torch.int32, device=dev)
        else:
            raise ValueError(f"unknown layout {layout!r}")
        self.layout = layout
        self.cell = float(cell)
        self._cindex = None  # (Grid, cell_off): cell index of the spatial storage order, built lazily
        self.ids, self.pos, self.caps = ids_t, pos, caps_t
        if n and int(ids_t.min()) < 0:
            raise ValueError("agent IDs must be non-negative")
        self.row_ptr = None
        self.col = None
        self.leader = torch.empty(n, dtype=torch.int32, device=dev)
        self.state = torch.full((n,), _lib.FOLLOWER, dtype=torch.uint8, device=dev)
        self._id_index = None
        self.resorts = 0            # resort() calls that changed the storage order
        self.last_resort_moved = 0  # rows the last resort() moved

    # ------------------------------------------------------------------ graph
    @property
    def n_edges(self) -> int:
        return 0 if self.col is None else int(self.col.numel())

    def build_graph(self, radius: float = 1.0):
        """Radius graph over the current storage order, built on the GPU (swarm_build_rgg)."""
        n, dev = self.n, self.device
        L = _lib.lib()
        row_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ne = ctypes.c_int64(0)
        with torch.cuda.device(dev):
            _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(self.pos) if n else None, float(radius),
                                         _lib.ptr(row_ptr), None, 0, ctypes.byref(ne), _lib.stream()))
            col = torch.empty(max(ne.value, 1), dtype=torch.int32, device=dev)
            _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(self.pos) if n else None, float(radius),
                                         _lib.ptr(row_ptr), _lib.ptr(col), col.numel(), ctypes.byref(ne),
                                         _lib.stream()))
        self.row_ptr, self.col = row_ptr, col[: ne.value]
        self._hear = None  # a radius graph is symmetric: its own transpose
        self._c16 = self._rp64 = self._pairs = None  # (their keys would miss anyway: frees the old graph's copies now)
        return self

    def set_graph(self, row_ptr, col):
        """CSR given over INPUT indices (as the caller numbered agents); relabelled to storage."""
        rp = np.asarray(row_ptr.cpu() if isinstance(row_ptr, torch.Tensor) else row_ptr, np.int64)
        cl = np.asarray(col.cpu() if isinstance(col, torch.Tensor) else col, np.int64)
        if rp[-1] >= 2**31:
            raise ValueError("graph has >= 2^31 edges; shard it (swarm_amd.dist)")
        perm = self.perm.cpu().numpy().astype(np.int64)
        if self.layout != "input" and self.n > 1:
            inv = np.empty(self.n, np.int64)
            inv[perm] = np.arange(self.n)
            deg = np.diff(rp)[perm]
            new_rp = np.zeros(self.n + 1, np.int64)
            new_rp[1:] = np.cumsum(deg)
            flat = np.repeat(rp[:-1][perm] - new_rp[:-1], deg) + np.arange(new_rp[-1])
            cl = inv[cl[flat]]
            rp = new_rp
        self.row_ptr = torch.as_tensor(rp.astype(np.int32), device=self.device)
        self.col = torch.as_tensor(cl.astype(np.int32), device=self.device)
        self._c16 = self._rp64 = self._pairs = None  # (their keys would miss anyway: frees the old graph's copies now)
        # hearers (transpose) CSR for the protocol's push marks: the same arrays when symmetric
        src = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(rp))
        fwd = np.sort(src * max(self.n, 1) + cl)
        bwd = np.sort(cl * max(self.n, 1) + src)
        if np.array_equal(fwd, bwd):
            self._hear = None
        else:
            order = np.argsort(cl, kind="stable")
            trp = np.zeros(self.n + 1, np.int64)
            trp[1:] = np.cumsum(np.bincount(cl, minlength=self.n))
            self._hear = (torch.as_tensor(trp.astype(np.int32), device=self.device),
                          torch.as_tensor(src[order].astype(np.int32), device=self.device))
        return self

    # ------------------------------------------------------------------ election
    def graph_compact(self) -> torch.Tensor | None:
        """16-bit columns of the (symmetric) neighbour graph (swarm_graph_compact: each neighbour as
        a delta from its row's 64-agent base), built on first use and rebuilt whenever row_ptr / col
        are replaced or modified in place; None when a delta does not fit (the int32 columns are
        used then) or the graph is directed."""
        if self.row_ptr is None or getattr(self, "_hear", None) is not None or not 0 < self.n < (1 << 30):
            return None
        # keyed on the tensor objects (held weakly) and their versions, not on addresses (_tensor_rec)
        cached = getattr(self, "_c16", None)
        if cached is None or not (_same_tensor(cached[0][0], self.row_ptr) and _same_tensor(cached[0][1], self.col)
                                  and cached[0][2:] == (self.n, self.col.numel())):
            key = (_tensor_rec(self.row_ptr), _tensor_rec(self.col), self.n, self.col.numel())
            c16 = torch.empty(max(self.col.numel(), 1), dtype=torch.int16, device=self.device)
            with torch.cuda.device(self.device):
                rc = _lib.lib().swarm_graph_compact(_lib.ctx(), self.n, _lib.ptr(self.row_ptr, torch.int32),
                                                    _lib.ptr(self.col, torch.int32) if self.col.numel() else None,
                                                    _lib.ptr(c16), _lib.stream())
            if rc == _lib.ERR_RANGE:
                c16 = None
            else:
                _lib.check(rc)
            self._c16 = cached = (key, c16)
        return cached[1]

    def graph_pairs(self):
        """The two-hop index of the (symmetric) neighbour graph for the election's pair rounds, as (rp2, col2)
        device tensors (swarm_graph_pairs_count / _fill: row v holds v's CSR row first, then the agents at
        exactly two hops, as 16-bit deltas from v & ~63), or None when it cannot be had: a directed graph, no
        edges, a delta that does not fit, a row longer than PAIR_ROW_CAP, 2^31 - 2^20 entries or more, or not
        enough device memory.  Built on first use and again whenever row_ptr / col are replaced or modified in
        place (keyed like graph_compact's columns); the refusal is cached too.  last_pairs_build_ms: the wall
        time of the last build."""
        if self.row_ptr is None or getattr(self, "_hear", None) is not None or not 0 < self.n < (1 << 30) \
                or self.n_edges == 0:
            return None
        cached = getattr(self, "_pairs", None)
        if cached is None or not (_same_tensor(cached[0][0], self.row_ptr) and _same_tensor(cached[0][1], self.col)
                                  and cached[0][2:] == (self.n, self.col.numel())):
            import time
            key = (_tensor_rec(self.row_ptr), _tensor_rec(self.col), self.n, self.col.numel())
            self._pairs = None  # the old index goes before the new one is allocated
            idx = None
            L = _lib.lib()
            t0 = time.perf_counter()
            with torch.cuda.device(self.device):
                try:
                    counts = torch.empty(self.n, dtype=torch.int32, device=self.device)
                    rc = L.swarm_graph_pairs_count(_lib.ctx(), self.n, _lib.ptr(self.row_ptr, torch.int32),
                                                   _lib.ptr(self.col, torch.int32), PAIR_ROW_CAP, _lib.ptr(counts),
                                                   _lib.stream())
                    if rc != _lib.ERR_RANGE:
                        _lib.check(rc)
                        rp2 = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
                        rp2[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
                        total = int(rp2[-1])
                        del counts
                        if 0 < total < _C16_EDGE_CAP:
                            rp2 = rp2.to(torch.int32)
                            col2 = torch.empty(total, dtype=torch.int16, device=self.device)
                            rc = L.swarm_graph_pairs_fill(_lib.ctx(), self.n, _lib.ptr(self.row_ptr, torch.int32),
                                                          _lib.ptr(self.col, torch.int32), _lib.ptr(rp2),
                                                          _lib.ptr(col2), _lib.stream())
                            if rc != _lib.ERR_RANGE:
                                _lib.check(rc)
                                idx = (rp2, col2)
                except torch.OutOfMemoryError:  # no room for the index: elect without pair rounds
                    idx = None
                torch.cuda.synchronize()
            self.last_pairs_build_ms = (time.perf_counter() - t0) * 1e3
            self._pairs = cached = (key, idx)
        return cached[1]

    def elect(self, mode: str = "frontier", max_rounds: int = 1 << 16, timed: bool = False,
              compact: bool = True, wide: bool | None = None, pairs: bool | None = None) -> ElectResult:
        """Contract E2 to convergence on the GPU (swarm_elect_compact with the graph's 16-bit
        columns when they fit; swarm_elect_directed when the neighbour lists are not symmetric).
        timed: per-kernel HIP events.  compact=False: the int32-column entry point swarm_elect
        (same results).  wide: int64 row offsets (swarm_elect_i64) -- chosen by itself for
        graphs of >= 2^30 edges unless their 16-bit columns fit (swarm_elect_compact then takes up
        to 2^31 - 2^20 edges on 32-bit offsets: C5's 100M agents on one GPU, ~1.6e9), True forces it.
        The 16-bit columns are graph_compact's, rebuilt whenever row_ptr / col change: the call passes
        SWARM_ELECT_TRUST_C16, so the library skips its device check of them (include/swarm.h).
        pairs: the frontier election's tail two rounds per launch through graph_pairs()'s index
        (swarm_elect_pairs; same results).  None: for swarms of at least SWARM_PAIR_MIN_AGENTS agents; True /
        False force it on / off.  Where the index cannot be had the election runs without (result.pair_launches
        is 0)."""
        if self.row_ptr is None:
            raise RuntimeError("no neighbour graph: call build_graph() or set_graph()")
        if wide is None:
            wide = self.n_edges >= (1 << 30) or self.n >= (1 << 30)
            if wide and self.n < (1 << 30) and self.n_edges < _C16_EDGE_CAP and compact \
                    and getattr(self, "_hear", None) is None and _c16_rounds():
                with torch.cuda.device(self.device):
                    wide = self.graph_compact() is None
        if wide:
            return self._elect_wide(mode, max_rounds, timed, compact)
        m = {"dense": _lib.ELECT_DENSE, "frontier": _lib.ELECT_FRONTIER}[mode] | (_lib.ELECT_TIMED if timed else 0)
        n = self.n
        rounds = ctypes.c_int32(0)
        cap = int(max_rounds)
        changes = np.empty(cap, np.int64)  # libswarm writes rounds 1..rounds_exec
        st = _lib.ElectStats()
        hear = getattr(self, "_hear", None)
        with torch.cuda.device(self.device):
            c16 = self.graph_compact() if (compact and hear is None) else None
            if pairs is None:
                pairs = n >= _pair_min_agents()
            idx = self.graph_pairs() if (pairs and c16 is not None and mode == "frontier" and _c16_rounds()) else None
            if idx is not None:  # symmetric graph, 16-bit columns, two-hop index: pair rounds in the tail
                rc = _lib.check(_lib.lib().swarm_elect_pairs(
                    _lib.ctx(), n, _lib.ptr(self.row_ptr, torch.int32), _lib.ptr(self.col, torch.int32),
                    _lib.ptr(c16), _lib.ptr(idx[0], torch.int32), _lib.ptr(idx[1], torch.int16),
                    _lib.ptr(self.ids, torch.int32), _lib.ptr(self.leader, torch.int32),
                    _lib.ptr(self.state, torch.uint8), cap, m | _TRUST_C16, ctypes.byref(rounds),
                    changes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st), _lib.stream()))
            elif c16 is not None:  # symmetric graph, 16-bit columns
                # graph_compact built them on this ctx from the current row_ptr / col (its cache key holds
                # their versions): the library skips its column check and edge-count read-back
                rc = _lib.check(_lib.lib().swarm_elect_compact(
                    _lib.ctx(), n, _lib.ptr(self.row_ptr, torch.int32), _lib.ptr(self.col, torch.int32),
                    _lib.ptr(c16), _lib.ptr(self.ids, torch.int32), _lib.ptr(self.leader, torch.int32),
                    _lib.ptr(self.state, torch.uint8), cap, m | _TRUST_C16, ctypes.byref(rounds),
                    changes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st), _lib.stream()))
            elif hear is None:  # symmetric graph: risers mark through their own rows
                rc = _lib.check(_lib.lib().swarm_elect(
                    _lib.ctx(), n, _lib.ptr(self.row_ptr, torch.int32), _lib.ptr(self.col, torch.int32),
                    _lib.ptr(self.ids, torch.int32), _lib.ptr(self.leader, torch.int32),
                    _lib.ptr(self.state, torch.uint8), cap, m, ctypes.byref(rounds),
                    changes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st), _lib.stream()))
            else:  # directed (from_agents / set_graph with asymmetric lists): mark the hearers
                rc = _lib.check(_lib.lib().swarm_elect_directed(
                    _lib.ctx(), n, _lib.ptr(self.row_ptr, torch.int32), _lib.ptr(self.col, torch.int32),
                    _lib.ptr(hear[0], torch.int32), _lib.ptr(hear[1], torch.int32) if hear[1].numel() else None,
                    _lib.ptr(self.ids, torch.int32), _lib.ptr(self.leader, torch.int32),
                    _lib.ptr(self.state, torch.uint8), cap, m, ctypes.byref(rounds),
                    changes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st), _lib.stream()))
        r = rounds.value
        res = ElectResult(r, changes[:r].copy(), self.leader, self.state, rc == _lib.OK,
                          st.rounds_launched, st.active_total, st.edges_total, st.dense_rounds,
                          st.bytes_total)
        res.changes_total = st.changes_total
        res.gather_ms, res.apply_ms, res.timed_launches = st.gather_ms, st.apply_ms, st.gather_launches
        res.sparse_ms, res.sparse_launches, res.sparse_bytes = st.sparse_ms, st.sparse_launches, st.sparse_bytes
        res.compact = c16 is not None  # the rounds read the 16-bit columns (2 of the 4 column bytes)
        res.wide = False               # 32-bit row offsets
        res.pair_launches = st.pair_launches  # launches that ran two rounds (0: no index, or never switched)
        return res

    def _elect_wide(self, mode: str, max_rounds: int, timed: bool, compact: bool = True) -> ElectResult:
        """swarm_elect_compact_i64 (16-bit columns when they fit) or swarm_elect_i64 over an int64
        copy of row_ptr (kept while row_ptr is unchanged)."""
        if getattr(self, "_hear", None) is not None:
            raise ValueError("int64 row offsets: symmetric neighbour graphs only (swarm_elect_i64)")
        cached = getattr(self, "_rp64", None)
        if cached is None or not (_same_tensor(cached[0][0], self.row_ptr) and cached[0][1] == self.n):
            self._rp64 = cached = ((_tensor_rec(self.row_ptr), self.n), self.row_ptr.to(torch.int64))
        rp64 = cached[1]
        m = {"dense": _lib.ELECT_DENSE, "frontier": _lib.ELECT_FRONTIER}[mode] | (_lib.ELECT_TIMED if timed else 0)
        rounds = ctypes.c_int32(0)
        cap = int(max_rounds)
        changes = np.empty(cap, np.int64)
        st = _lib.ElectStats()
        with torch.cuda.device(self.device):
            c16 = self.graph_compact() if compact else None
            rc = _lib.check(_lib.lib().swarm_elect_compact_i64(
                _lib.ctx(), self.n, _lib.ptr(rp64, torch.int64), _lib.ptr(self.col, torch.int32),
                _lib.ptr(c16) if c16 is not None else None,
                _lib.ptr(self.ids, torch.int32), _lib.ptr(self.leader, torch.int32),
                _lib.ptr(self.state, torch.uint8), cap, m, ctypes.byref(rounds),
                changes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st), _lib.stream()))
        r = rounds.value
        res = ElectResult(r, changes[:r].copy(), self.leader, self.state, rc == _lib.OK,
                          st.rounds_launched, st.active_total, st.edges_total, st.dense_rounds,
                          st.bytes_total)
        res.changes_total = st.changes_total
        res.gather_ms, res.apply_ms, res.timed_launches = st.gather_ms, st.apply_ms, st.gather_launches
        res.sparse_ms, res.sparse_launches, res.sparse_bytes = st.sparse_ms, st.sparse_launches, st.sparse_bytes
        # the int64-offset DENSE rounds read the int32 columns (elect.hip launch_dense_round takes
        # col16 only with 32-bit offsets): only the frontier's sparse rounds read the 16-bit ones
        res.compact = c16 is not None and mode == "frontier"
        res.wide = True
        res.pair_launches = 0
        return res

    # ------------------------------------------------------------------ allocation
    def id_index(self) -> torch.Tensor | None:
        """id -> storage index table (None if IDs are too sparse for a dense table); built on first use and
        again whenever self.ids is replaced or modified in place."""
        if self.n and (self._id_index is None or not _same_tensor(getattr(self, "_id_index_key", None), self.ids)):
            self._id_index = None
            span = int(self.ids.max()) + 1
            if span <= 4 * self.n + 1024:
                t = torch.full((span,), -1, dtype=torch.int32, device=self.device)
                t[self.ids.long()] = torch.arange(self.n, dtype=torch.int32, device=self.device)
                self._id_index = t
                self._id_index_key = _tensor_rec(self.ids)
        return self._id_index

    def _indexable(self, mode, claim_thr, u_scale) -> bool:
        """The binned round can use the storage order's cell index: spatial layout, a finite claim
        radius spanning <= 16 index rows (else swarm_allocate bins by hashed cells)."""
        if self.layout != "spatial" or self.n < 2 or mode == "dense" or not (claim_thr > 0 and u_scale > 0):
            return False
        rp = (u_scale / claim_thr - 1.0) * (1 + 1e-9) + 1e-12
        return rp > 0 and np.floor(2.0 * rp / self.cell) + 2 <= 16  # index cells are >= self.cell

    def _cell_index(self):
        """(Grid, cell_off) of the storage order (swarm_cell_index), built once; the allocation
        verifies it on the device every call and drops it when positions have moved.  None when
        the current positions are no longer in cell order (after physics_step moved agents across
        cells): allocate() then bins by hashed cells, and the index is tried again only after
        the positions change again (self._cindex = False marks 'not indexable' for the position
        tensor and version in self._cindex_bad)."""
        if self._cindex is False:
            if self._indexed_pos("_cindex_bad"):
                return None
            self._cindex = None
        if self._cindex is None:
            L, g, nc = _lib.lib(), _lib.Grid(), ctypes.c_int64(0)
            _lib.check(L.swarm_cell_index(_lib.ctx(), self.n, _lib.ptr(self.pos), self.cell, ctypes.byref(g), None, 0,
                                          ctypes.byref(nc), _lib.stream()))
            off = torch.empty(nc.value + 1, dtype=torch.int32, device=self.device)
            rc = L.swarm_cell_index(_lib.ctx(), self.n, _lib.ptr(self.pos), self.cell, ctypes.byref(g),
                                    _lib.ptr(off), off.numel(), ctypes.byref(nc), _lib.stream())
            if rc == _lib.ERR_ARG and "not in cell order" in _lib.last_error():
                self._cindex, self._cindex_bad = False, (self.pos, self.pos._version)
                return None
            _lib.check(rc)
            self._cindex = (g, off)
            # the positions it indexed: the tensor object itself (held, so its storage cannot be handed to
            # another tensor) and its version; allocate trusts the index while both are unchanged
            self._cindex_key = (self.pos, self.pos._version)
        return self._cindex

    def _indexed_pos(self, attr="_cindex_key") -> bool:
        """self.pos is the very tensor, at the same version, that the key `attr` recorded."""
        k = getattr(self, attr, None)
        return k is not None and k[0] is self.pos and k[1] == self.pos._version

    def allocate(self, tx, ty, treq, *, winner=None, util=None, claim_thr: float = 20.0,
                 hysteresis: float = 5.0, u_scale: float = 100.0, mode: str = "auto") -> AllocResult:
        """One allocation round over t tasks (swarm_allocate).  winner/util = existing claims."""
        if winner is None and util is None and mode == "auto":
            r = self._allocate_again(tx, ty, treq, claim_thr, hysteresis, u_scale)
            if r is not None:
                return r
        dev = self.device
        tpos = self._task_pos(tx, ty)
        tq = _to(treq, torch.int8, dev)
        t = tq.numel()
        # no claim table: winner / util are outputs only (the indexed call initialises them on the device)
        fresh = winner is None and util is None
        w = (torch.empty(t, dtype=torch.int32, device=dev) if winner is None
             else _to(winner, torch.int32, dev).clone())
        u = (torch.empty(t, dtype=torch.float64, device=dev) if util is None
             else _to(util, torch.float64, dev).clone())
        # libswarm zeroes won and writes nclaim / nmsg for every task (one buffer for both)
        won = torch.empty(self.n, dtype=torch.int32, device=dev)
        nc_nm = torch.empty((2, t), dtype=torch.int64, device=dev)
        nclaim, nmsg = nc_nm[0], nc_nm[1]
        idx = self.id_index()
        st = _lib.AllocStats()
        m = {"auto": _lib.ALLOC_AUTO, "binned": _lib.ALLOC_BINNED, "dense": _lib.ALLOC_DENSE}[mode]
        L = _lib.lib()
        # every tensor below is this call's or the Swarm's own (contiguous, on dev): raw pointers
        p = _fast_ptr
        with torch.cuda.device(dev):
            ci = self._cell_index() if self._indexable(mode, claim_thr, u_scale) else None
            rc = _lib.ERR_STALE
            if ci is not None:  # spatial storage order: no binning pass (swarm_allocate_indexed_ex)
                # the index is trusted while self.pos is the tensor and version it was built from (the
                # device staleness check runs otherwise); the claim table is updated in place: keep
                # the caller's for a stale-index retry
                trusted = self._indexed_pos()
                flags = (_lib.ALLOC_TRUST_INDEX if trusted else 0) | (_lib.ALLOC_FRESH_CLAIMS if fresh else 0)
                w0 = None if winner is None or trusted else w.clone()
                u0 = None if util is None or trusted else u.clone()
                rc = L.swarm_allocate_indexed_ex(
                    _lib.ctx(), self.n, p(self.ids), p(self.pos), p(self.caps),
                    ctypes.byref(ci[0]), p(ci[1]), t, p(tpos), p(tq), float(claim_thr),
                    float(hysteresis), float(u_scale), flags, p(w), p(u), p(won), p(idx),
                    0 if idx is None else idx.numel(), p(nclaim), p(nmsg), ctypes.byref(st),
                    _lib.stream())
                if rc == _lib.OK and trusted and fresh and mode == "auto" and isinstance(treq, torch.Tensor) \
                        and tq is treq:
                    # the same call again (same task tensors and versions, same trusted index, same
                    # swarm arrays) needs none of the above: _allocate_again replays it from here
                    self._again = ((tx, ty, treq, (tx._version, ty._version, treq._version), self.pos,
                                    self.pos._version, self.ids, self.caps, (claim_thr, hysteresis, u_scale),
                                    torch.cuda.current_device()),
                                   (self.n, self.ids.data_ptr(), self.pos.data_ptr(), self.caps.data_ptr(),
                                    ctypes.byref(ci[0]), ci[1].data_ptr(), t, tpos.data_ptr(), tq.data_ptr(),
                                    float(claim_thr), float(hysteresis), float(u_scale), flags),
                                   (idx.data_ptr() if idx is not None else None, 0 if idx is None else idx.numel()),
                                   (ci, tpos, idx))
                if rc == _lib.ERR_STALE:  # positions moved since the index: bin them this call
                    self._cindex = None  # rebuilt next call if they are still in cell order
                    w.copy_(w0) if w0 is not None else w.fill_(-1)
                    u.copy_(u0) if u0 is not None else u.zero_()
                else:
                    _lib.check(rc)
            if rc == _lib.ERR_STALE:
                if ci is None and fresh:
                    w.fill_(-1)
                    u.zero_()
                _lib.check(L.swarm_allocate(
                    _lib.ctx(), self.n, p(self.ids), p(self.pos), p(self.caps), t,
                    p(tpos), p(tq), float(claim_thr), float(hysteresis), float(u_scale), m,
                    p(w), p(u), p(won), p(idx),
                    0 if idx is None else idx.numel(), p(nclaim), p(nmsg),
                    ctypes.byref(st), _lib.stream()))
        stats = {k: getattr(st, k) for k, _ in _lib.AllocStats._fields_}
        return AllocResult(w, u, won, nclaim, nmsg, stats)

    def _allocate_again(self, tx, ty, treq, claim_thr, hysteresis, u_scale):
        """The previous fresh, trusted-index allocation repeated (the same task tensors at the same
        versions, the same swarm arrays and position version, the same thresholds, on the same device):
        one libswarm call with its arguments kept from that call -- none of allocate()'s per-call Python
        (task stacking, index checks, device context, pointer validation).  None when anything differs."""
        c = getattr(self, "_again", None)
        if c is None:
            return None
        k = c[0]
        if not (k[0] is tx and k[1] is ty and k[2] is treq and k[4] is self.pos and k[6] is self.ids
                and k[7] is self.caps and k[3] == (tx._version, ty._version, treq._version)
                and k[5] == self.pos._version and k[8] == (claim_thr, hysteresis, u_scale)
                and k[9] == torch.cuda.current_device() and c[3][0] is self._cindex
                and c[3][2] is self._id_index):
            return None
        a = c[1]
        t, n = a[6], self.n
        # the four outputs carved from ONE allocation (one caching-allocator call instead of four):
        # util (f64), nclaim + nmsg (i64), winner (i32), won (i32), each 8-byte aligned
        buf = torch.empty(24 * t + 4 * t + 4 * n + 8, dtype=torch.uint8, device=self.device)
        b0 = buf.data_ptr()
        u = buf[:8 * t].view(torch.float64)
        nc_nm = buf[8 * t:24 * t].view(torch.int64).view(2, t)
        w = buf[24 * t:28 * t].view(torch.int32)
        o_won = (28 * t + 7) & ~7
        won = buf[o_won:o_won + 4 * n].view(torch.int32)
        st = _lib.AllocStats()
        _lib.check(_lib.lib().swarm_allocate_indexed_ex(_lib.ctx(), *a, b0 + 24 * t, b0, b0 + o_won, *c[2],
                                                        b0 + 8 * t, b0 + 16 * t, ctypes.byref(st), _lib.stream()))
        return AllocResult(w, u, won, nc_nm[0], nc_nm[1], {k_: getattr(st, k_) for k_, _ in _lib.AllocStats._fields_})

    def _task_pos(self, tx, ty) -> torch.Tensor:
        """(t, 2) float64 task positions on the device.  When tx / ty are float64 device tensors the
        stacked copy is kept and reused while both are unchanged (the same tensor objects at the
        same version counters): a caller that allocates over the same tasks every step pays no
        stacking kernel."""
        dev = self.device
        if isinstance(tx, torch.Tensor) and isinstance(ty, torch.Tensor) and tx.dtype == ty.dtype == torch.float64 \
                and tx.device == ty.device == dev:
            # the SAME tensor objects (held by the cache, so their storage cannot be recycled) at
            # the same version counters
            c = getattr(self, "_tpos_cache", None)
            if c is not None and c[0] is tx and c[1] is ty and c[2] == (tx._version, ty._version):
                return c[3]
            tpos = torch.stack([tx, ty], 1).contiguous()
            self._tpos_cache = (tx, ty, (tx._version, ty._version), tpos)
            return tpos
        return torch.stack([_to(tx, torch.float64, dev), _to(ty, torch.float64, dev)], 1).contiguous()

    def auction(self, tx, ty, treq, *, eps: float = 0.1, claim_thr: float = 20.0, u_scale: float = 100.0,
                max_rounds: int = 1 << 20) -> AuctionResult:
        """Auction allocation over the admissible pairs (swarm_auction; SURVEY §8f f4, the north
        star's auction price update): one task per agent, highest bid wins, ties to the lowest
        ID.  No reference counterpart; parity against oracle.auction."""
        dev = self.device
        tpos = torch.stack([_to(tx, torch.float64, dev), _to(ty, torch.float64, dev)], 1).contiguous()
        tq = _to(treq, torch.int8, dev)
        t = tq.numel()
        owner = torch.empty(max(t, 1), dtype=torch.int32, device=dev)
        price = torch.empty(max(t, 1), dtype=torch.float32, device=dev)
        assigned = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        rounds = ctypes.c_int32(0)
        bidders = np.zeros(int(max_rounds), np.int64)
        st = _lib.AuctionStats()
        with torch.cuda.device(dev):
            rc = _lib.check(_lib.lib().swarm_auction(
                _lib.ctx(), self.n, _lib.ptr(self.ids), _lib.ptr(self.pos), _lib.ptr(self.caps), t,
                _lib.ptr(tpos), _lib.ptr(tq), float(claim_thr), float(u_scale), float(eps), int(max_rounds),
                _lib.ptr(owner), _lib.ptr(price), _lib.ptr(assigned), ctypes.byref(rounds),
                bidders.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st), _lib.stream()))
        r = rounds.value
        stats = {k: getattr(st, k) for k, _ in _lib.AuctionStats._fields_}
        return AuctionResult(owner[:t], price[:t], assigned[: self.n], r, bidders[:r].copy(), rc == _lib.OK, stats)

    # ------------------------------------------------------------------ physics
    def leader_index(self, leader: torch.Tensor | None = None) -> torch.Tensor:
        """Storage index of each FOLLOWER's leader (-1 for leaders / unknown IDs), from the
        election's leader IDs (self.leader after elect())."""
        leader = self.leader if leader is None else _to(leader, torch.int32, self.device)
        out = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
        idx = self.id_index()
        if idx is None or self.n == 0:
            srt, order = torch.sort(self.ids.long())
            pos = torch.searchsorted(srt, leader.long()).clamp(max=max(self.n - 1, 0))
            hit = srt[pos] == leader.long()
            cand = torch.where(hit, order[pos].int(), out)
        else:
            ok = (leader >= 0) & (leader < idx.numel())
            cand = torch.where(ok, idx[leader.clamp(0, idx.numel() - 1).long()], out)
        return torch.where(self.state == _lib.FOLLOWER, cand, out).contiguous()

    def obstacle_field(self, obstacles, velocities=None) -> ObstacleField:
        """An ObstacleField of the (m, 3) [x, y, r] list on this swarm's device (contract O1, DESIGN 4j;
        swarm_obstacle_field_create).  The list is copied.  Built on the host, once; every `obstacles=`
        parameter accepts the field.  SwarmError: ERR_ARG for a non-finite entry or footprints without a finite
        extent, ERR_RANGE for more than 2^26 (cell, obstacle) pairs.
        velocities: (m, 2) makes it a moving field (contract O2; swarm_obstacle_field_create_moving):
        the sensed calls rebuild its lists on the device every tick and advance every obstacle by v * dt after
        the tick's physics; ERR_ARG for a non-finite velocity, ERR_RANGE when the pair bound from the radii
        exceeds 2^26.  See ObstacleField."""
        return ObstacleField(obstacles, self.device, velocities)

    def physics_step(self, obstacles=None, *, sensors=None, leader_index=None, dt: float = 0.1,
                     max_speed: float = 5.0, steps: int = 1, sense_radius: float | None = None) -> dict:
        """`steps` synchronous _update_physics steps (agent.py:94-181) of every agent, in place on
        self.pos (contract P1; swarm_physics_step).  obstacles: (m, 3) [x, y, r]; sensors:
        (row_ptr, col) over storage indices (default: the neighbour graph); leader_index:
        default self.leader_index().  Velocity / target state lives on the Swarm.
        sense_radius: every step senses its neighbours from that step's positions instead (contract
        S1; swarm_physics_run_sensed, all steps in one call): the result of build_graph(sense_radius)
        + physics_step(steps=1) repeated, bit for bit, with no graph built and self.row_ptr /
        self.col untouched.  `sensors` must then be None.  The dict gains "steps_done"; a step whose
        cell windows are too dense raises SwarmError (ERR_RANGE) with the steps run before it in
        self.last_steps_done."""
        if sense_radius is not None and sensors is not None:
            raise ValueError("sense_radius senses the neighbours itself: sensors must be None")
        if sense_radius is None:
            _no_moving_field(obstacles, "physics_step without sense_radius")
        dev, n = self.device, self.n
        if not hasattr(self, "vel"):
            self.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            self.target = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            self.has_target = torch.zeros(n, dtype=torch.uint8, device=dev)
        obs_m, obs_ptr, _obs_keep = _obstacle_args(obstacles, dev)
        if sense_radius is not None:
            li = self.leader_index() if leader_index is None else _to(leader_index, torch.int32, dev)
            sing, done = ctypes.c_int64(0), ctypes.c_int32(0)
            p = lambda t: _lib.ptr(t) if n else None  # noqa: E731
            with torch.cuda.device(dev):
                rc = _lib.lib().swarm_physics_run_sensed(
                    _lib.ctx(), n, p(self.ids), p(self.state), p(li), p(self.pos), p(self.vel), p(self.target),
                    p(self.has_target), obs_m, obs_ptr, float(sense_radius),
                    int(steps), float(dt), float(max_speed), ctypes.byref(done), ctypes.byref(sing), _lib.stream())
            self.last_steps_done = done.value
            if done.value:
                self._cindex = None  # agents moved: the storage order is no longer their cell order
            _lib.check(rc)
            return {"singular": sing.value, "steps_done": done.value}
        rp, col = sensors if sensors is not None else (self.row_ptr, self.col)
        if rp is None:
            raise RuntimeError("no sensor graph: pass sensors=(row_ptr, col) or build_graph()")
        rp, col = _to(rp, torch.int32, dev), _to(col, torch.int32, dev)
        li = self.leader_index() if leader_index is None else _to(leader_index, torch.int32, dev)
        other = torch.empty_like(self.pos)
        sing = ctypes.c_int64(0)
        total = 0
        with torch.cuda.device(dev):
            for _ in range(int(steps)):
                _lib.check(_lib.lib().swarm_physics_step(
                    _lib.ctx(), n, _lib.ptr(self.ids), _lib.ptr(self.state), _lib.ptr(li), _lib.ptr(self.pos),
                    _lib.ptr(other), _lib.ptr(self.vel), _lib.ptr(self.target), _lib.ptr(self.has_target),
                    obs_m, obs_ptr, _lib.ptr(rp), _lib.ptr(col) if col.numel() else None,
                    float(dt), float(max_speed), ctypes.byref(sing), _lib.stream()))
                total += sing.value
                self.pos, other = other, self.pos
                self._cindex = None  # agents moved: the storage order is no longer their cell order
        return {"singular": total}

    # ------------------------------------------------------------------ timer FSM (f2)
    def _storage(self, a, dtype):
        """Per-agent array in INPUT order -> storage order on the device."""
        t = _to(a, dtype, self.device)
        if t.numel() != self.n:
            raise ValueError(f"expected {self.n} values, got {t.numel()}")
        return t[self.perm.long()].contiguous() if self.layout != "input" else t

    def protocol_reset(self, tick_off=None, last_hb=None):
        """Every agent as SwarmAgent.__init__ leaves it (agent.py:31-39): FOLLOWER, no leader,
        no leader position, alive, nothing in flight; last_heartbeat_time = last_hb (input
        order, default 0.0 = the clock at tick 0); tick_off: each agent's tick-counter phase
        (input order, default 0 = lock-step).  Tick counter restarts at 0."""
        n, dev = self.n, self.device
        self._drop_agent_life()
        z = lambda dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
        self.state.fill_(_lib.FOLLOWER)
        self.leader.fill_(-1)
        self.fsm = dict(last_hb=z(torch.float64) if last_hb is None else self._storage(last_hb, torch.float64),
                        wait_start=z(torch.float64), delay=z(torch.float64),
                        leader_pos=torch.zeros((n, 2), dtype=torch.float32, device=dev),
                        has_leader_pos=z(torch.uint8), alive=torch.ones(n, dtype=torch.uint8, device=dev),
                        outbox=torch.zeros(2 * n, dtype=torch.uint8, device=dev))
        self.tick_off = z(torch.int32) if tick_off is None else self._storage(tick_off, torch.int32)
        self.fsm_tick = 0
        return self

    def protocol_run(self, ticks: int, *, kill_ticks=(), dt: float = 0.1, timeout: float = 3.0,
                     jitter: float = 0.2, seed: int = 0, mode: str = "hybrid", pull_frac: float = 0.125,
                     traffic: bool = False) -> np.ndarray:
        """Advance the timer FSM + election handlers `ticks` ticks under contract T1
        (swarm_protocol_run; agent.py:66-80, 217-289), messages along the neighbour graph.
        kill_ticks: absolute ticks at whose start every alive LEADER dies.  Returns counts
        (ticks x 4): alive LEADERs, alive ELECTION_WAITs, ACCLAIM senders, HEARTBEAT senders.
        mode "push": senders mark their hearers and only marked agents scan their row; "pull":
        every agent scans its row every tick; "hybrid": push, but a tick in which a workgroup's
        senders exceed pull_frac x its share of the agents (a timeout wave) has the next tick pull
        (swarm_protocol_run_ex).  Same results.
        traffic: count what the ticks touched (self.fsm_traffic: 8 int64, see include/swarm.h)."""
        if self.row_ptr is None:
            raise RuntimeError("no neighbour graph: call build_graph() or set_graph()")
        if not hasattr(self, "fsm"):
            self.protocol_reset()
        f = self.fsm
        fs = _lib.Fsm(*[_lib.ptr(t) if self.n else None for t in
                        (self.state, self.leader, f["last_hb"], f["wait_start"], f["delay"], f["leader_pos"],
                         f["has_leader_pos"], f["alive"], f["outbox"])])
        kt = np.ascontiguousarray(np.asarray(kill_ticks, np.int64))
        if mode not in ("push", "pull", "hybrid"):
            raise ValueError(f"unknown mode {mode!r}")
        h = getattr(self, "_hear", None) or (self.row_ptr, self.col)
        hear = (None, None) if mode == "pull" or self.n == 0 else \
            (_lib.ptr(h[0], torch.int32), _lib.ptr(h[1], torch.int32) if h[1].numel() else None)
        counts = np.zeros((int(ticks), 4), np.int64)
        tr = np.zeros(8, np.int64)
        self._agent_life_current()
        agent_events = self._agent_events(ticks)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().swarm_protocol_run_ex(
                _lib.ctx(), self.n, _lib.ptr(self.ids) if self.n else None, _lib.ptr(self.pos) if self.n else None,
                _lib.ptr(self.row_ptr, torch.int32), _lib.ptr(self.col, torch.int32) if self.n_edges else None,
                *hear, _lib.ptr(self.tick_off) if self.n else None, ctypes.byref(fs), self.fsm_tick, int(ticks),
                float(dt), float(timeout), float(jitter), ctypes.c_uint64(int(seed)),
                kt.ctypes.data_as(ctypes.c_void_p) if kt.size else None, kt.size,
                float(pull_frac) if mode == "hybrid" else -1.0, counts.ctypes.data_as(ctypes.c_void_p),
                tr.ctypes.data_as(ctypes.c_void_p) if traffic else None, _lib.stream()))
        if traffic:
            self.fsm_traffic = tr
        self.fsm_tick += int(ticks)
        self.last_agent_events = agent_events
        return counts

    # ------------------------------------------------------------------ agent lifetimes (U1-J)
    def _drop_agent_life(self):
        life = self.__dict__.pop("agent_life", None)
        if life is not None:
            life["finalizer"]()

    def _attach_agent_life(self, boot, death, apply_rule):
        """The handle of the windows (input order) on the current alive / tick_off tensors, in storage order;
        apply_rule: the set-time rule at self.fsm_tick (swarm_agent_life_set)."""
        import weakref
        n = self.n
        order = slice(None) if self.layout == "input" else self.perm.cpu().numpy().astype(np.int64)
        bs, ds = np.ascontiguousarray(boot[order]), np.ascontiguousarray(death[order])
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if n else None  # noqa: E731
        alive, tick_off = self.fsm["alive"], self.tick_off
        old = getattr(self, "agent_life", None)
        if apply_rule and old is not None and old["alive"] is alive and old["tick_off"] is tick_off:
            # the handle stands on the current tensors: new windows and the set-time rule in one call
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().swarm_agent_life_set(old["ctx"], old["handle"], n, hp(bs), hp(ds),
                                                           int(self.fsm_tick), _lib.stream()))
            old["boot"], old["death"] = boot.copy(), death.copy()
            return
        self._drop_agent_life()
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            ctx = _lib.ctx()
            _lib.check(_lib.lib().swarm_agent_life_create(ctx, n, hp(bs), hp(ds), _lib.ptr(alive) if n else None,
                                                          _lib.ptr(tick_off) if n else None, ctypes.byref(handle)))
            self.agent_life = dict(boot=boot.copy(), death=death.copy(), handle=handle, ctx=ctx, alive=alive,
                                   tick_off=tick_off,
                                   finalizer=weakref.finalize(self, _destroy_agent_life, ctx, handle))
            if apply_rule:
                _lib.check(_lib.lib().swarm_agent_life_set(ctx, handle, n, hp(bs), hp(ds), int(self.fsm_tick),
                                                           _lib.stream()))

    def _agent_life_current(self):
        """The lifetimes' handle names the alive / tick_off tensors the next call passes: rebuilt on the current
        ones when either has been replaced (resort() replaces both, with the storage order)."""
        life = getattr(self, "agent_life", None)
        if life is not None and (life["alive"] is not self.fsm["alive"] or life["tick_off"] is not self.tick_off):
            self._attach_agent_life(life["boot"], life["death"], apply_rule=False)

    def _agent_events(self, ticks) -> np.ndarray:
        """(ticks x 2) the agents that boot and die at each of the next `ticks` ticks (swarm_agent_life_events)."""
        ev = np.zeros((int(ticks), 2), np.int64)
        life = getattr(self, "agent_life", None)
        if life is not None and ticks:
            _lib.check(_lib.lib().swarm_agent_life_events(life["ctx"], life["handle"], int(self.fsm_tick), int(ticks),
                                                          ev.ctypes.data_as(ctypes.c_void_p)))
        return ev

    def set_agent_lifetimes(self, boot_tick, death_tick):
        """Agent lifetimes (contract U1-J; swarm_agent_life_create / _set), allowed between calls: agent i
        (input order) is up at tick t -- the absolute ticks the loops count -- iff boot_tick[i] <= t <
        death_tick[i].  (n,) ints or scalars; None for boot_tick is tick 0, for death_tick never; both None removes
        the lifetimes.  With self.fsm_tick = T the last tick run, agents with boot > T or death <= T lose their alive
        flag now; the others keep the flag they have.  At the start of tick t of protocol_run and of every
        update_loop*, after the leader kill of kill_ticks: agents with death == t die as a kill_ticks victim does
        (alive = 0, everything else stays, what they sent during t-1 is still heard); then agents with boot == t
        become a fresh SwarmAgent constructed at the clock of tick t-1 -- FOLLOWER, no leader, last_hb = (t-1) dt,
        their own tick counter 1 at tick t, velocity 0, no target, nothing in flight, on a task board every task
        OPEN again and an empty claim table -- at the position they stand at.  A boot of an agent that is up is a
        restart; a second window set after a death is a rebirth.  A run cut into calls is the single run; a refused
        call fires nothing.  The loops' dicts carry "agent_events" (ticks x 2: booted, died per tick);
        protocol_run leaves it in self.last_agent_events.  protocol_reset() drops the lifetimes.  ValueError: a boot
        tick outside [0, 2^31), a negative death tick, a wrong shape."""
        life = _agent_lifetimes(boot_tick, death_tick, self.n)
        if life is None:
            self._drop_agent_life()
            return self
        if not hasattr(self, "fsm"):
            self.protocol_reset()
        self._attach_agent_life(*life, apply_rule=True)
        return self

    def agent_lifetimes(self):
        """(boot_tick, death_tick), each a (n,) int64 numpy array in input order; None without lifetimes."""
        life = getattr(self, "agent_life", None)
        return None if life is None else (life["boot"].copy(), life["death"].copy())

    def agents_up(self, tick=None) -> np.ndarray:
        """(n,) bool, input order: the agents whose window holds `tick` (default: the next tick to run); all of
        them without lifetimes.  (An agent killed at a kill tick is in its window and dead: fsm["alive"].)"""
        life = getattr(self, "agent_life", None)
        if life is None:
            return np.ones(self.n, bool)
        t = getattr(self, "fsm_tick", 0) + 1 if tick is None else int(tick)
        return (life["boot"] <= t) & (t < life["death"])

    # ------------------------------------------------------------------ coupled update loop (U1)
    def _motion_state(self):
        """vel / target / has_target, created as physics_step creates them."""
        if not hasattr(self, "vel"):
            n, dev = self.n, self.device
            self.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            self.target = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            self.has_target = torch.zeros(n, dtype=torch.uint8, device=dev)

    def _target_rows(self, index):
        """Storage rows of the agents `index` names in INPUT numbering (None: every agent, input order)."""
        if index is not None:
            idx = np.atleast_1d(np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index))
            if idx.ndim != 1 or idx.dtype.kind not in "iu":
                raise ValueError("index must be a 1-D array of agent indices (input order)")
            if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.n):
                raise ValueError(f"index out of range for {self.n} agents")
        else:
            idx = None
        if self.layout == "input":
            return None if idx is None else torch.as_tensor(idx.astype(np.int64), device=self.device)
        inv = torch.empty(self.n, dtype=torch.int64, device=self.device)
        inv[self.perm.long()] = torch.arange(self.n, dtype=torch.int64, device=self.device)
        return inv if idx is None else inv[torch.as_tensor(idx.astype(np.int64), device=self.device)]

    def set_target(self, x, y, index=None):
        """SwarmAgent.set_target (agent.py:56-57), batched: agent index[k] (INPUT numbering; None = every
        agent, in input order) gets the target (x[k], y[k]); scalars go to every agent named."""
        count = self.n if index is None else int(np.atleast_1d(np.asarray(
            index.cpu() if isinstance(index, torch.Tensor) else index)).shape[0])
        xy = []
        for name, v in (("x", x), ("y", y)):
            a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, np.float64)
            if a.ndim == 0:
                a = np.full(count, float(a))
            if a.shape != (count,):
                raise ValueError(f"{name}: expected {count} values, got shape {tuple(a.shape)}")
            xy.append(a)
        rows = self._target_rows(index)
        self._motion_state()
        t = torch.as_tensor(np.stack(xy, 1), device=self.device)
        if rows is None:
            self.target.copy_(t)
            self.has_target.fill_(1)
        else:
            self.target[rows] = t
            self.has_target[rows] = 1
        return self

    def clear_target(self, index=None):
        """target = None for the agents `index` names (INPUT numbering; None = every agent): they stop
        where they are until a leader position gives them a slot again."""
        rows = self._target_rows(index)
        self._motion_state()
        if rows is None or index is None:
            self.target.zero_()
            self.has_target.zero_()
        else:
            self.target[rows] = 0.0
            self.has_target[rows] = 0
        return self

    def update_loop(self, ticks: int, *, obstacles=None, sensors=None, kill_ticks=(), dt: float = 0.1,
                    timeout: float = 3.0, jitter: float = 0.2, seed: int = 0, max_speed: float = 5.0,
                    mode: str = "hybrid", pull_frac: float = 0.125, trace_every: int = 0) -> dict:
        """`ticks` ticks of the reference's update_loop (agent.py:67-81) for every agent, in one call on the
        GPU (contract U1; swarm_update_loop): each tick protocol_run's tick, then a physics step in which
        every alive agent uses its own FSM state -- a FOLLOWER steers to the V slot behind the leader
        position its last accepted heartbeat carried (f32, up to ten ticks old), an ELECTION_WAIT agent or
        a new LEADER keeps its last target, dead agents stay frozen.  A heartbeat carries the position its
        sender had when it packed it, one physics step before the tick that receives it.
        obstacles: (m, 3) [x, y, r]; sensors: (row_ptr, col) over storage indices, fixed for the call
        (default: the neighbour graph); the other keywords as protocol_run / physics_step.  Uses self.fsm /
        self.fsm_tick as protocol_run does and advances self.fsm_tick, so calls chain into one run.
        self.pos_prev holds the positions one tick before self.pos (what the heartbeats in flight carry);
        it is kept from the previous update_loop call while self.pos is still that call's tensor, untouched
        since -- when anything else has moved or replaced self.pos, or there was no previous call, it
        starts as a copy of self.pos.
        Returns {"counts": (ticks x 4) as protocol_run, "singular": zero distances over all ticks} and,
        with trace_every = k > 0, "trace": (ticks // k, n, 2) positions after every k-th tick of the call,
        storage order.  update_loop_sensed senses the separation neighbours anew every tick instead."""
        _no_moving_field(obstacles, "update_loop")
        return self._update_loop(ticks, None, obstacles, sensors, kill_ticks, dt, timeout, jitter, seed, max_speed,
                                 mode, pull_frac, trace_every)

    def update_loop_sensed(self, ticks: int, sense_radius: float, *, obstacles=None, sensors=None, kill_ticks=(),
                           dt: float = 0.1, timeout: float = 3.0, jitter: float = 0.2, seed: int = 0,
                           max_speed: float = 5.0, mode: str = "hybrid", pull_frac: float = 0.125,
                           trace_every: int = 0) -> dict:
        """update_loop with every tick's separation neighbours sensed from that tick's positions (contract
        U1-S; swarm_update_loop_sensed; the reference's simulator calls update_sensors before every tick): the
        result of "radius graph of the current storage positions at sense_radius, then update_loop(1,
        sensors=that graph)" repeated, bit for bit, with no graph built.  The message graph self.row_ptr /
        self.col is fixed and untouched.  Keywords, self.fsm / self.fsm_tick / self.pos_prev and the returned
        dict as update_loop; the calls of the two chain into one run.  `sensors` is update_loop's keyword and
        has no meaning here: anything but None raises ValueError before the device is touched.
        All or nothing: a tick whose cell windows are too dense raises SwarmError (ERR_RANGE) with the
        absolute tick in self.last_refused_tick (-1 after a call that went through), and positions, motion
        state, FSM and self.fsm_tick are what they were before the call (run in chunks to keep the progress
        up to such a tick)."""
        if sensors is not None:
            raise ValueError("update_loop_sensed senses the neighbours itself: sensors must be None")
        return self._update_loop(ticks, float(sense_radius), obstacles, None, kill_ticks, dt, timeout, jitter, seed,
                                 max_speed, mode, pull_frac, trace_every)

    def update_loop_radio(self, ticks: int, radio_radius: float, sense_radius: float, *, obstacles=None,
                          kill_ticks=(), dt: float = 0.1, timeout: float = 3.0, jitter: float = 0.2, seed: int = 0,
                          max_speed: float = 5.0, trace_every: int = 0, loss: float = 0.0,
                          loss_seed: int = 0) -> dict:
        """update_loop_sensed with who hears whom re-sensed every tick as well (contract U1-R;
        swarm_update_loop_radio): at tick t an alive agent hears every other agent within radio_radius of it in
        the positions at the start of the tick -- the snapshot the tick's sensors read -- and receives what
        those sent during tick t-1 in ascending storage index; a heartbeat still carries the position its
        sender packed a tick earlier.  An agent that has moved out of its leader's range stops hearing it,
        times out and re-elects.  The result of "radius graph of the current storage positions at
        radio_radius as the message graph, then update_loop_sensed(1, sense_radius)" repeated, bit for bit,
        with no graph built: the swarm needs no neighbour graph, and self.row_ptr / self.col are untouched
        when it has one.  Keywords, self.fsm / self.fsm_tick / self.pos_prev, the returned dict, the
        all-or-nothing refusal of a too-dense tick and self.last_refused_tick as update_loop_sensed; the calls
        of the three loops chain into one run.
        loss > 0: a lossy channel (contract U1-L; swarm_update_loop_channel).  At absolute tick t the link
        from an in-range sender to a receiver is dropped with probability `loss`, decided by a hash of
        (loss_seed, t, sender ID, receiver ID) -- the same in every layout and however the run is cut into
        calls -- and a dropped link delivers nothing of what the sender sent during tick t-1.  The two
        directions of a pair are decided independently.  The dict then gains "link_counts" (ticks x 2): per
        tick the election links (alive receiver, in-range sender with an ACCLAIM or a HEARTBEAT) and how many
        of them were dropped.  loss outside [0, 1] or NaN raises ValueError; with the default 0.0 the call is
        the loss-free one, whatever loss_seed is."""
        radio_radius, sense_radius = float(radio_radius), float(sense_radius)
        for name, r in (("radio_radius", radio_radius), ("sense_radius", sense_radius)):
            if not (r > 0.0 and np.isfinite(r)):
                raise ValueError(f"{name} must be positive and finite, got {r}")
        return self._update_loop(ticks, sense_radius, obstacles, None, kill_ticks, dt, timeout, jitter, seed,
                                 max_speed, "pull", 0.125, trace_every, radio_radius=radio_radius,
                                 channel=_channel(loss, loss_seed))

    # ------------------------------------------------------------------ task update loop (U1-T)
    def set_tasks(self, tx, ty=None, treq=None):
        """A fresh task board shared by every agent (each reference agent's `tasks` dict holding all T tasks,
        T <= 64): every task OPEN at every agent, every claim table empty, no claim or conflict in flight.
        tx / ty: task positions; treq: required capability bit per task, -1 = none (default).  A
        tasks_from_dict result (task_ids, tx, ty, treq) may be given as the only argument; its task_ids are
        kept in self.task_ids.  update_loop_tasks then runs the board; T and treq are checked there, by the
        library (SwarmError ERR_ARG, nothing written)."""
        ids = None
        if ty is None and isinstance(tx, tuple) and len(tx) == 4:
            ids, tx, ty, treq = tx
        tx = np.atleast_1d(np.asarray(tx, np.float64))
        ty = np.atleast_1d(np.asarray(ty, np.float64))
        if tx.ndim != 1 or tx.shape != ty.shape:
            raise ValueError("tx and ty must be 1-D arrays of one length")
        T, n, dev = int(tx.shape[0]), self.n, self.device
        tq = np.full(T, -1, np.int8) if treq is None else np.atleast_1d(np.asarray(treq)).astype(np.int64)
        if tq.shape != (T,):
            raise ValueError(f"treq: expected {T} values, got shape {tuple(tq.shape)}")
        if T and (int(tq.min()) < -128 or int(tq.max()) > 127):
            raise ValueError("treq must fit a signed byte (the library accepts -1 .. 31)")
        z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731  (u64 words)
        self.tasks = dict(T=T, tpos=torch.as_tensor(np.stack([tx, ty], 1), device=dev).contiguous(),
                          treq=torch.as_tensor(tq.astype(np.int8), device=dev), status_lo=z(n), status_hi=z(n),
                          claim_out=z(2 * n), conflict_out=z(2 * n),
                          tab_winner=torch.full((n, T), -1, dtype=torch.int32, device=dev),
                          tab_util=torch.zeros((n, T), dtype=torch.float32, device=dev))
        self.task_ids = np.arange(T, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        return self

    def update_loop_tasks(self, ticks: int, radio_radius: float, sense_radius: float, *, obstacles=None,
                          kill_ticks=(), dt: float = 0.1, timeout: float = 3.0, jitter: float = 0.2, seed: int = 0,
                          max_speed: float = 5.0, trace_every: int = 0, loss: float = 0.0,
                          loss_seed: int = 0) -> dict:
        """update_loop_radio with the reference's task logic run every tick on the board of set_tasks
        (contract U1-T; swarm_update_loop_tasks; agent.py:292-336): an agent claims a task on the tick it is
        within reach of it (U > 20 at the tick's snapshot) and marks it TENTATIVE; only a LEADER that hears
        the claim arbitrates, in its own claim table, with the 5.0 hysteresis; its TASK_CONFLICT messages set
        the task ASSIGNED at the winner and LOCKED at everyone else who hears them, the last one heard (in
        ascending storage index) deciding; a claim no leader hears is lost.  Keywords, self.fsm /
        self.fsm_tick / self.pos_prev, the all-or-nothing refusal (every task array restored as well) and the
        chaining with the other three loops as update_loop_radio; claims and conflicts in flight carry over
        between calls.  Returns update_loop_radio's dict plus "task_counts" (ticks x 3: TASK_CLAIMs sent,
        claims handled by a LEADER, TASK_CONFLICT messages sent) and "guard", the evaluated (agent, task)
        pairs whose utility is so close to 20 that libm pow arithmetic could have decided differently.
        loss / loss_seed: update_loop_radio's lossy channel; a dropped link delivers neither the sender's
        election packets nor its TASK_CLAIMs nor its TASK_CONFLICTs, and "link_counts" is returned as there."""
        channel = _channel(loss, loss_seed)
        if not hasattr(self, "tasks"):
            raise RuntimeError("no task board: call set_tasks() first")
        radio_radius, sense_radius = float(radio_radius), float(sense_radius)
        for name, r in (("radio_radius", radio_radius), ("sense_radius", sense_radius)):
            if not (r > 0.0 and np.isfinite(r)):
                raise ValueError(f"{name} must be positive and finite, got {r}")
        return self._update_loop(ticks, sense_radius, obstacles, None, kill_ticks, dt, timeout, jitter, seed,
                                 max_speed, "pull", 0.125, trace_every, radio_radius=radio_radius, tasks=self.tasks,
                                 channel=channel)

    def task_status(self) -> torch.Tensor:
        """(n, T) uint8 status codes (indices into STATUS_NAMES), storage order."""
        b = self.tasks
        k = torch.arange(b["T"], dtype=torch.int64, device=self.device)[None, :]
        lo, hi = (b["status_lo"][:, None] >> k) & 1, (b["status_hi"][:, None] >> k) & 1
        return (lo | (hi << 1)).to(torch.uint8)

    def task_tables(self):
        """Every agent's task_claims as dense tables, storage order: (winner (n, T) int32, -1 = no entry;
        utility (n, T) float32)."""
        return self.tasks["tab_winner"], self.tasks["tab_util"]

    def write_back_tasks(self, agents, task_ids=None):
        """Status strings into every agent object's `tasks` dict and its task_claims (agent.py:41-44), as the
        loop left them; agents in input order, task_ids[k]: the dict key of board task k (default:
        self.task_ids)."""
        task_ids = self.task_ids if task_ids is None else task_ids
        st = self.to_input_order(self.task_status())
        w, u = (self.to_input_order(t) for t in self.task_tables())
        for i, a in enumerate(agents):
            for k, tid in enumerate(task_ids):
                task = a.tasks.get(int(tid))
                if task is not None:
                    task["status"] = STATUS_NAMES[st[i, k]]
            a.task_claims = {int(tid): {"winner": int(w[i, k]), "utility": float(u[i, k])}
                             for k, tid in enumerate(task_ids) if w[i, k] >= 0}

    # ------------------------------------------------------------------ task loop on boards of any size (U1-B)
    def set_task_board(self, tx, ty=None, treq=None, *, status_slots: int = 16, table_slots: int = 16,
                       velocities=None, open_tick=None, close_tick=None):
        """set_tasks for a board of up to 2^24 tasks (contract U1-B; swarm_board_create): every task OPEN at
        every agent, every claim table empty, nothing in flight, the per-agent state sparse -- status_slots
        non-OPEN statuses and table_slots claim-table entries per agent at most, each in [1, 4096].  An agent
        that needs one more makes update_loop_board refuse the call (grow_board, then repeat it).  Arguments as
        set_tasks, a tasks_from_dict result included; the positions and treq are checked here, by the library
        (SwarmError ERR_ARG).  The 64-task board of set_tasks is a separate one and is left alone.
        velocities ((T, 2), finite): a moving board (contract U1-M; swarm_board_create_moving) -- after every tick
        of update_loop_board each task advances by fl(v * dt), the cell grid is rebuilt on the device before every
        tick, and a claim is heard with the positions it was sent with; board_positions() reads them back.
        open_tick / close_tick ((T,) ints or scalars; either one makes the board a moving one, at rest unless
        velocities are given): task lifetimes (contract U1-A; set_board_lifetimes)."""
        import weakref
        ids = None
        if ty is None and isinstance(tx, tuple) and len(tx) == 4:
            ids, tx, ty, treq = tx
        tx = np.atleast_1d(np.asarray(tx, np.float64))
        ty = np.atleast_1d(np.asarray(ty, np.float64))
        if tx.ndim != 1 or tx.shape != ty.shape:
            raise ValueError("tx and ty must be 1-D arrays of one length")
        T, n, dev = int(tx.shape[0]), self.n, self.device
        tq = np.full(T, -1, np.int8) if treq is None else np.atleast_1d(np.asarray(treq)).astype(np.int64)
        if tq.shape != (T,):
            raise ValueError(f"treq: expected {T} values, got shape {tuple(tq.shape)}")
        if T and (int(tq.min()) < -128 or int(tq.max()) > 127):
            raise ValueError("treq must fit a signed byte (the library accepts -1 .. 31)")
        ks, kt = int(status_slots), int(table_slots)
        for name, k in (("status_slots", ks), ("table_slots", kt)):
            if not 1 <= k <= _lib.BOARD_MAX_SLOTS:
                raise ValueError(f"{name} must be in [1, {_lib.BOARD_MAX_SLOTS}], got {k}")
        vel = None if velocities is None else _board_velocities(velocities, T)
        life = _board_lifetimes(open_tick, close_tick, T)
        if life is not None and vel is None:
            vel = np.zeros((T, 2))
        old = getattr(self, "board", None)
        if old is not None:
            old["finalizer"]()
        desc, handle = _lib.BoardDesc(), ctypes.c_void_p()
        with torch.cuda.device(dev):
            tpos = torch.as_tensor(np.stack([tx, ty], 1), device=dev).contiguous()
            rq = torch.as_tensor(tq.astype(np.int8), device=dev)
            ctx = _lib.ctx()
            if vel is None:
                _lib.check(_lib.lib().swarm_board_create(ctx, T, _lib.ptr(tpos) if T else None,
                                                         _lib.ptr(rq) if T else None, ctypes.byref(handle),
                                                         ctypes.byref(desc), _lib.stream()))
            else:
                dv = torch.as_tensor(vel, device=dev)
                _lib.check(_lib.lib().swarm_board_create_moving(ctx, T, _lib.ptr(tpos) if T else None,
                                                                _lib.ptr(rq) if T else None,
                                                                _lib.ptr(dv) if T else None, ctypes.byref(handle),
                                                                ctypes.byref(desc), _lib.stream()))
        e = lambda rows, k: torch.full((rows, k), -1, dtype=torch.int32, device=dev)  # noqa: E731
        self.board = dict(T=T, handle=handle, ctx=ctx, Ks=ks, Kt=kt, moving=vel is not None,
                          info={k: getattr(desc, k) for k, _ in _lib.BoardDesc._fields_},
                          status=e(n, ks), tab_task=e(n, kt), tab_winner=e(n, kt),
                          tab_util=torch.zeros((n, kt), dtype=torch.float32, device=dev),
                          claim_out=e(2 * n, ks), conflict_out=e(2 * n, kt),
                          finalizer=weakref.finalize(self, _destroy_board, ctx, handle))
        self.board_task_ids = np.arange(T, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.last_board_overflow = None
        if life is not None:
            self._set_lifetimes(*life)
        return self

    def _set_lifetimes(self, lo, hi):
        b = self.board
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().swarm_board_set_lifetimes(
                b["ctx"], b["handle"], None if lo is None else lo.ctypes.data_as(ctypes.c_void_p),
                None if hi is None else hi.ctypes.data_as(ctypes.c_void_p), _lib.stream()))
        b["life"] = None if lo is None else (lo.copy(), hi.copy())

    def set_board_lifetimes(self, open_tick, close_tick):
        """Task lifetimes for the moving board of set_task_board (contract U1-A, DESIGN 4q;
        swarm_board_set_lifetimes), allowed between calls: task k is present at tick t -- the absolute ticks
        update_loop_board counts and loss= hashes -- iff open_tick[k] <= t < close_tick[k].  (T,) ints or scalars;
        None for open_tick is tick 0, for close_tick never; both None removes the lifetimes.  Only present tasks are
        offered; a conflict about an absent task writes nothing; at the tick a task closes, and at the first tick
        after this call, the status entries of absent tasks leave every agent's row (their slots are free again),
        while claim tables keep theirs.  ValueError: a negative tick, open > close, a wrong shape."""
        if not hasattr(self, "board"):
            raise RuntimeError("no task board: call set_task_board() first")
        b = self.board
        if not b.get("moving"):
            raise RuntimeError("the task board does not move: lifetimes need set_task_board(..., velocities=...) "
                               "or set_task_board(..., open_tick=..., close_tick=...)")
        life = _board_lifetimes(open_tick, close_tick, b["T"])
        self._set_lifetimes(*(life if life is not None else (None, None)))
        return self

    def board_lifetimes(self):
        """(open_tick, close_tick), each a (T,) int64 numpy array read back from the board
        (swarm_board_lifetimes); None when the board has no lifetimes."""
        b = self.board
        lo, hi = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.lib().swarm_board_lifetimes(b["handle"], ctypes.byref(lo), ctypes.byref(hi)))
        if not lo.value:
            return None
        out = np.zeros(b["T"], np.int64), np.zeros(b["T"], np.int64)
        if b["T"]:
            with torch.cuda.device(self.device):
                torch.cuda.current_stream().synchronize()
                for a, p in zip(out, (lo, hi)):
                    _lib.copy_to_host(a, p)
        return out

    def board_present(self, tick=None) -> np.ndarray:
        """(T,) bool: the tasks present at `tick` (default: the next tick to run); all of them on a board without
        lifetimes."""
        b = self.board
        life = b.get("life")
        if life is None:
            return np.ones(b["T"], bool)
        t = getattr(self, "fsm_tick", 0) + 1 if tick is None else int(tick)
        return (life[0] <= t) & (t < life[1])

    def _placeable_board(self):
        if not hasattr(self, "board"):
            raise RuntimeError("no task board: call set_task_board() first")
        b = self.board
        if not b.get("moving") or b.get("life") is None:
            raise RuntimeError("placing needs a task board with lifetimes: set_task_board(..., open_tick=..., "
                               "close_tick=...) or set_board_lifetimes()")
        return b

    def board_last_tick(self) -> int:
        """The last tick update_loop_board ran on the board (swarm_board_last_tick); -1: none yet."""
        t = ctypes.c_int64(-1)
        _lib.check(_lib.lib().swarm_board_last_tick(self.board["handle"], ctypes.byref(t)))
        return int(t.value)

    def board_free_slots(self, tick=None) -> np.ndarray:
        """The slots place_board_tasks may fill (contract U1-P.1, the quiet rule), ascending: those whose task was
        absent at `tick` and at the tick before it -- tick: the last tick run (the default), since a place is
        checked against that one."""
        b = self._placeable_board()
        last = getattr(self, "fsm_tick", 0) if tick is None else int(tick)
        lo, hi = b["life"]
        return np.flatnonzero((hi < last) | (lo > last) | (lo == hi))

    def place_board_tasks(self, index, tx, ty, treq=None, *, velocities=None, open_tick=None, close_tick=None,
                          keep_tables: bool = False, task_ids=None) -> dict:
        """New tasks into the slots of closed ones (contract U1-P; swarm_board_place), between
        update_loop_board calls: slot index[j] of the board takes position (tx[j], ty[j]), requirement treq[j]
        (default none), velocity velocities[j] (default at rest) and the window [open_tick[j], close_tick[j]) --
        open_tick defaults to the next tick to run, close_tick to never; scalars or one per slot.  Only a slot of
        board_free_slots() can be placed.  Every claim-table entry about a placed slot is removed at every agent
        unless keep_tables (the reference re-adding the same task id: the old winner's hysteresis then applies).
        task_ids[j]: the dict key write_back_board gives the new task (default: unchanged).
        -> {"purged": table entries removed, "next_tick": the tick the next update_loop_board call starts with}.
        ValueError: shapes, ticks and values the library would refuse, found before the device is touched;
        SwarmError ERR_ARG: what only the library sees, nothing changed."""
        b = self._placeable_board()
        T = b["T"]
        idx = np.atleast_1d(np.asarray(index))
        if idx.size == 0:
            idx = idx.astype(np.int64)
        if idx.ndim != 1 or idx.dtype.kind not in "iu":
            raise ValueError("index must be a 1-D array of integer slots")
        idx = idx.astype(np.int64)
        m = int(idx.shape[0])
        if m and (int(idx.min()) < 0 or int(idx.max()) >= T):
            raise ValueError(f"index: a slot outside [0, {T})")
        if len(np.unique(idx)) != m:
            raise ValueError("index: a slot is listed twice")
        tx = np.atleast_1d(np.asarray(tx, np.float64))
        ty = np.atleast_1d(np.asarray(ty, np.float64))
        if tx.shape != (m,) or ty.shape != (m,):
            raise ValueError(f"tx and ty: expected {m} values each")
        if not (np.isfinite(tx).all() and np.isfinite(ty).all()):
            raise ValueError("task positions must be finite")
        tq = np.full(m, -1, np.int64) if treq is None else np.atleast_1d(np.asarray(treq)).astype(np.int64)
        if tq.shape != (m,):
            raise ValueError(f"treq: expected {m} values, got shape {tuple(tq.shape)}")
        if m and (int(tq.min()) < -1 or int(tq.max()) > 31):
            raise ValueError("treq must be in [-1, 31]")
        vel = None if velocities is None else _board_velocities(velocities, m)
        last = getattr(self, "fsm_tick", 0)
        lo, hi = _board_lifetimes(last + 1 if open_tick is None else open_tick, close_tick, m)
        if m and int(lo.min()) <= last:
            raise ValueError(f"task {int(np.argmax(lo <= last))} opens at or before the last tick run ({last})")
        ids = None
        if task_ids is not None:
            ids = np.atleast_1d(np.asarray(task_ids, np.int64))
            if ids.shape != (m,):
                raise ValueError(f"task_ids: expected {m} keys")
        free = np.zeros(T, bool)
        free[self.board_free_slots()] = True
        if m and not free[idx].all():
            raise ValueError(f"slot {int(idx[np.argmin(free[idx])])} is not free: its task was present at one of the "
                             "last two ticks (board_free_slots() lists the free ones)")
        purged = ctypes.c_int64(0)
        if m:
            i32 = np.ascontiguousarray(idx.astype(np.int32))
            pos = np.ascontiguousarray(np.stack([tx, ty], 1))
            rq = np.ascontiguousarray(tq.astype(np.int8))
            p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            state = _lib.BoardState(b["Ks"], b["Kt"], None, _lib.ptr(b["status"]), _lib.ptr(b["tab_task"]),
                                    _lib.ptr(b["tab_winner"]), _lib.ptr(b["tab_util"]), _lib.ptr(b["claim_out"]),
                                    _lib.ptr(b["conflict_out"]))
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().swarm_board_place(
                    b["ctx"], b["handle"], self.n, ctypes.byref(state), m, p(i32), p(pos), p(rq), p(vel), p(lo),
                    p(hi), _lib.PLACE_KEEP_TABLES if keep_tables else 0, ctypes.byref(purged), _lib.stream()))
            b["life"][0][idx], b["life"][1][idx] = lo, hi
            if ids is not None:
                old = self.board_task_ids[idx]
                b.setdefault("left_ids", set()).update(int(k) for k in old[old != ids])
                b["left_ids"].difference_update(int(k) for k in ids)
                self.board_task_ids = self.board_task_ids.copy()
                self.board_task_ids[idx] = ids
        return {"purged": int(purged.value), "next_tick": last + 1}

    def update_loop_board(self, ticks: int, radio_radius: float, sense_radius: float, *, obstacles=None,
                          kill_ticks=(), dt: float = 0.1, timeout: float = 3.0, jitter: float = 0.2, seed: int = 0,
                          max_speed: float = 5.0, trace_every: int = 0, loss: float = 0.0,
                          loss_seed: int = 0) -> dict:
        """update_loop_tasks on the board of set_task_board (contract U1-B; swarm_update_loop_board): the same
        tick, handler for handler, the same keywords, lossy channel and obstacle fields included, and the same
        dict.  An agent that needs more status or table slots than the board was set with makes the call all or
        nothing, like a too-dense tick: SwarmError ERR_RANGE, self.last_refused_tick is the tick and
        self.last_board_overflow (kind "status" or "table", one such agent in input order); grow_board() and the
        same call then run it.  Sparse rows that are not canonical (set by hand) are refused with ERR_ARG."""
        channel = _channel(loss, loss_seed)
        if not hasattr(self, "board"):
            raise RuntimeError("no task board: call set_task_board() first")
        radio_radius, sense_radius = float(radio_radius), float(sense_radius)
        for name, r in (("radio_radius", radio_radius), ("sense_radius", sense_radius)):
            if not (r > 0.0 and np.isfinite(r)):
                raise ValueError(f"{name} must be positive and finite, got {r}")
        return self._update_loop(ticks, sense_radius, obstacles, None, kill_ticks, dt, timeout, jitter, seed,
                                 max_speed, "pull", 0.125, trace_every, radio_radius=radio_radius, board=self.board,
                                 channel=channel)

    def board_positions(self):
        """The board's two position lists by task index, (cur, lag), each a (T, 2) float64 numpy array: a static
        board's positions twice; a moving board's (contract U1-M) current positions and those one advance behind
        (equal until the first tick)."""
        b = self.board
        T = b["T"]
        cur, lag = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.lib().swarm_board_positions(b["handle"], ctypes.byref(cur), ctypes.byref(lag)))
        out = np.zeros((T, 2)), np.zeros((T, 2))
        if T:
            with torch.cuda.device(self.device):
                torch.cuda.current_stream().synchronize()
                for a, p in zip(out, (cur, lag)):
                    _lib.copy_to_host(a, p)
        return out

    def set_board_velocities(self, v):
        """New velocities ((T, 2), finite) for the moving board of set_task_board(velocities=...); neither position
        list changes (swarm_board_set_velocities)."""
        b = self.board
        if not b.get("moving"):
            raise RuntimeError("the task board does not move: call set_task_board(..., velocities=...)")
        vel = _board_velocities(v, b["T"])
        with torch.cuda.device(self.device):
            dv = torch.as_tensor(vel, device=self.device)
            _lib.check(_lib.lib().swarm_board_set_velocities(b["ctx"], b["handle"], _lib.ptr(dv) if b["T"] else None,
                                                             _lib.stream()))
        return self

    def board_status(self) -> torch.Tensor:
        """(n, status_slots) int32 sparse status rows, storage order: task << 2 | code (1 TENTATIVE, 2 LOCKED,
        3 ASSIGNED) ascending by task, -1 behind the last entry."""
        return self.board["status"]

    def board_tables(self):
        """Every agent's task_claims as sparse rows, storage order: (task (n, table_slots) int32 ascending, -1 =
        empty; winner int32; utility float32)."""
        b = self.board
        return b["tab_task"], b["tab_winner"], b["tab_util"]

    def board_dense(self):
        """The board state as update_loop_tasks' dense arrays, for small n x T, storage order: (status (n, T)
        uint8 codes, winner (n, T) int32 with -1 = no entry, utility (n, T) float32)."""
        b, n, dev = self.board, self.n, self.device
        T = b["T"]
        status = torch.zeros((n, T), dtype=torch.uint8, device=dev)
        winner = torch.full((n, T), -1, dtype=torch.int32, device=dev)
        util = torch.zeros((n, T), dtype=torch.float32, device=dev)
        st, tt = b["status"], b["tab_task"]
        rows = torch.arange(n, device=dev)[:, None]
        m = st >= 0
        status[rows.expand_as(st)[m], (st[m] >> 2).long()] = (st[m] & 3).to(torch.uint8)
        m = tt >= 0
        at = (rows.expand_as(tt)[m], tt[m].long())
        winner[at] = b["tab_winner"][m]
        util[at] = b["tab_util"][m]
        return status, winner, util

    def grow_board(self, status_slots=None, table_slots=None):
        """More slots per agent (never fewer): the rows padded with empty slots, so that a refused
        update_loop_board call can be repeated."""
        b = self.board
        ks = b["Ks"] if status_slots is None else int(status_slots)
        kt = b["Kt"] if table_slots is None else int(table_slots)
        for name, k, have in (("status_slots", ks, b["Ks"]), ("table_slots", kt, b["Kt"])):
            if not have <= k <= _lib.BOARD_MAX_SLOTS:
                raise ValueError(f"{name} must be in [{have}, {_lib.BOARD_MAX_SLOTS}], got {k}")

        def pad(t, k, fill):
            out = torch.full((t.shape[0], k), fill, dtype=t.dtype, device=t.device)
            out[:, :t.shape[1]] = t
            return out
        for key, k, fill in (("status", ks, -1), ("claim_out", ks, -1), ("tab_task", kt, -1), ("tab_winner", kt, -1),
                             ("tab_util", kt, 0), ("conflict_out", kt, -1)):
            b[key] = pad(b[key], k, fill)
        b["Ks"], b["Kt"] = ks, kt
        return self

    def write_back_board(self, agents, task_ids=None):
        """write_back_tasks for the board of set_task_board: the non-OPEN statuses and the task_claims as the
        loop left them; agents in input order, task_ids[k]: the dict key of board task k (default: the
        tasks_from_dict keys given to set_task_board)."""
        task_ids = self.board_task_ids if task_ids is None else task_ids
        st = self.to_input_order(self.board_status())
        tt, tw, tu = (self.to_input_order(t) for t in self.board_tables())
        # (contract U1-A) the tasks absent at the last tick run are no entry of an agent's `tasks`
        gone = [int(task_ids[k]) for k in np.flatnonzero(~self.board_present(getattr(self, "fsm_tick", 0)))] \
            if self.board.get("life") is not None else ()
        # (contract U1-P) ... nor are the keys whose slot place_board_tasks gave to another task
        gone = list(gone) + sorted(self.board.get("left_ids", ()))
        for i, a in enumerate(agents):
            for key in gone:
                a.tasks.pop(key, None)
            for e in st[i][st[i] >= 0]:
                task = a.tasks.get(int(task_ids[int(e) >> 2]))
                if task is not None:
                    task["status"] = STATUS_NAMES[int(e) & 3]
            a.task_claims = {int(task_ids[int(k)]): {"winner": int(w), "utility": float(u)}
                             for k, w, u in zip(tt[i], tw[i], tu[i]) if k >= 0 and w >= 0}

    # ------------------------------------------------------------------ task census (U1-C)
    def board_census(self, *, alive_only: bool = False, holders: bool = False) -> dict:
        """What the swarm decided, per task of the board of set_task_board (contract U1-C; swarm_board_census):
        a dict of ten device tensors of length T -- "tentative", "locked", "assigned", "tables" (int32 counts of
        agents with that status of the task / with a claim-table entry for it), "holder_lo", "holder_hi" (the
        lowest / highest agent ID among the ASSIGNED holders, -1 without one), "winner_lo", "winner_hi" (the
        lowest / highest winner the table entries name; the tables agree iff they are equal; -1 without an
        entry), "best_winner", "best_util" (the entry with the highest utility, ties to the lowest winner; -1 and
        0.0 without one).  Bit-exact, whatever the storage order.  alive_only: only agents with fsm["alive"] are
        counted.  holders: also "holders", every (task, agent ID) pair with status ASSIGNED as an (m, 2) int32
        tensor sorted by (task, ID).  Nothing of the swarm is changed; rows set by hand that are not canonical
        are refused (SwarmError ERR_ARG)."""
        if not hasattr(self, "board"):
            raise RuntimeError("no task board: call set_task_board() first")
        b, mask = self.board, self._census_mask(alive_only)
        if b["status"].shape[0] != self.n:
            raise ValueError("the task board was set for another number of agents")
        p = lambda t: _lib.ptr(t) if self.n else None  # noqa: E731
        bs = _lib.BoardState(b["Ks"], b["Kt"], None, *[p(b[k]) for k in ("status", "tab_task", "tab_winner",
                                                                        "tab_util")], None, None)

        def call(ctx, ids, mask, out, pairs, cap, total):
            return _lib.lib().swarm_board_census(ctx, self.n, ids, b["handle"], ctypes.byref(bs), mask, out, pairs,
                                                 cap, total, _lib.stream())
        return self._census(b["T"], call, mask, holders)

    def task_census(self, *, alive_only: bool = False, holders: bool = False) -> dict:
        """board_census for the 64-task board of set_tasks (swarm_tasks_census): the same dict."""
        if not hasattr(self, "tasks"):
            raise RuntimeError("no task board: call set_tasks() first")
        b, mask = self.tasks, self._census_mask(alive_only)
        if b["status_lo"].shape[0] != self.n:
            raise ValueError("the task board was set for another number of agents")
        p = lambda k: _lib.ptr(b[k]) if b[k].numel() else None  # noqa: E731

        def call(ctx, ids, mask, out, pairs, cap, total):
            return _lib.lib().swarm_tasks_census(ctx, self.n, ids, b["T"], p("status_lo"), p("status_hi"),
                                                 p("tab_winner"), p("tab_util"), mask, out, pairs, cap, total,
                                                 _lib.stream())
        return self._census(b["T"], call, mask, holders)

    def _census_mask(self, alive_only):
        if not alive_only:
            return None
        if not hasattr(self, "fsm"):
            raise RuntimeError("alive_only needs the protocol state: call protocol_reset() or run a loop first")
        return self.fsm["alive"]

    def _census(self, T, call, mask, holders) -> dict:
        """The output tensors and the holder buffer of a census call: T + 1024 pairs at first, the call repeated
        once with the exact count when the total came back larger."""
        dev, n = self.device, self.n
        res = {k: torch.empty(T, dtype=torch.float32 if k == "best_util" else torch.int32, device=dev)
               for k in _lib.CENSUS_FIELDS}
        pairs = torch.empty((0, 2), dtype=torch.int32, device=dev)
        if T:  # (a board without tasks has nothing to count: ten empty tensors, no call)
            out = _lib.Census(*[_lib.ptr(res[k]) for k in _lib.CENSUS_FIELDS])
            total, cap = ctypes.c_int64(0), (T + 1024 if holders else 0)
            with torch.cuda.device(dev):
                for _ in range(2):
                    buf = torch.empty((cap, 2), dtype=torch.int32, device=dev) if holders else None
                    _lib.check(call(_lib.ctx(), _lib.ptr(self.ids) if n else None,
                                    _lib.ptr(mask) if mask is not None and n else None, ctypes.byref(out),
                                    _lib.ptr(buf), cap, ctypes.byref(total)))
                    if not holders or total.value <= cap:
                        break
                    cap = total.value
            if holders:
                pairs = buf[:total.value]
        if holders:
            order = torch.argsort(pairs[:, 0].long() * (1 << 31) + pairs[:, 1].long())
            res["holders"] = pairs[order].contiguous()
        return res

    def _update_loop(self, ticks, sense_radius, obstacles, sensors, kill_ticks, dt, timeout, jitter, seed,
                     max_speed, mode, pull_frac, trace_every, radio_radius=None, tasks=None, channel=None,
                     board=None) -> dict:
        """update_loop (sense_radius None: the `sensors` lists, fixed), update_loop_sensed,
        update_loop_radio (radio_radius given: no message graph), update_loop_tasks (tasks: the board) and
        update_loop_board (board: the sparse one); channel: (loss, loss_seed) with loss > 0 -- the two radio
        loops through swarm_update_loop_channel."""
        ticks, trace_every = int(ticks), int(trace_every)
        if mode not in ("push", "pull", "hybrid"):
            raise ValueError(f"unknown mode {mode!r}")
        if ticks < 0:
            raise ValueError("ticks must not be negative")
        if trace_every < 0:
            raise ValueError("trace_every must not be negative")
        if self.row_ptr is None and radio_radius is None:
            raise RuntimeError("no neighbour graph: call build_graph() or set_graph()")
        dev, n = self.device, self.n
        if not hasattr(self, "fsm"):
            self.protocol_reset()
        self._motion_state()
        if sense_radius is None:
            srp, scol = (self.row_ptr, self.col) if sensors is None else \
                (_to(sensors[0], torch.int32, dev), _to(sensors[1], torch.int32, dev))
            if srp.numel() != n + 1:
                raise ValueError(f"sensors: row_ptr needs {n + 1} entries, got {srp.numel()}")
        obs_m, obs_ptr, _obs_keep = _obstacle_args(obstacles, dev)
        k = getattr(self, "_pos_prev_key", None)
        if k is None or k[0] is not self.pos or k[1] != self.pos._version or not hasattr(self, "pos_prev"):
            self.pos_prev = self.pos.clone()
        f = self.fsm
        fs = _lib.Fsm(*[_lib.ptr(t) if n else None for t in
                        (self.state, self.leader, f["last_hb"], f["wait_start"], f["delay"], f["leader_pos"],
                         f["has_leader_pos"], f["alive"], f["outbox"])])
        self._agent_life_current()
        agent_events = self._agent_events(ticks)
        kt = np.ascontiguousarray(np.asarray(kill_ticks, np.int64))
        if radio_radius is None:
            h = getattr(self, "_hear", None) or (self.row_ptr, self.col)
            hear = (None, None) if mode == "pull" or n == 0 else \
                (_lib.ptr(h[0], torch.int32), _lib.ptr(h[1], torch.int32) if h[1].numel() else None)
        counts = np.zeros((ticks, 4), np.int64)
        frames = ticks // trace_every if trace_every else 0
        trace = torch.empty((frames, n, 2), dtype=torch.float64, device=dev) if trace_every else None
        sing = ctypes.c_int64(0)
        p = lambda t: _lib.ptr(t) if n else None  # noqa: E731
        refused = ctypes.c_int64(-1)
        with torch.cuda.device(dev):
            graph = () if radio_radius is not None else \
                (_lib.ptr(self.row_ptr, torch.int32), _lib.ptr(self.col, torch.int32) if self.n_edges else None, *hear)
            run = (p(self.tick_off), ctypes.byref(fs), self.fsm_tick, ticks, float(dt), float(timeout), float(jitter),
                   ctypes.c_uint64(int(seed)), kt.ctypes.data_as(ctypes.c_void_p) if kt.size else None, kt.size)
            motion = (p(self.vel), p(self.target), p(self.has_target), obs_m, obs_ptr)
            head = (_lib.ctx(), n, p(self.ids), p(self.pos), p(self.pos_prev), *graph, *run,
                    *(() if radio_radius is not None else (float(pull_frac) if mode == "hybrid" else -1.0,)), *motion)
            tail = (float(max_speed), _lib.ptr(trace) if frames and n else None, trace_every,
                    counts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(sing))
            tk, task_counts, guard = None, None, ctypes.c_int64(0)
            if tasks is not None:
                T = tasks["T"]
                if any(tasks[k].shape[0] != size for k, size in (("status_lo", n), ("claim_out", 2 * n))):
                    raise ValueError("the task board was set for another number of agents")
                tp = lambda k: _lib.ptr(tasks[k]) if tasks[k].numel() else None  # noqa: E731
                tk = _lib.Tasks(T, tp("tpos"), tp("treq"), p(self.caps) if T else None,
                                *[tp(k) for k in ("status_lo", "status_hi", "claim_out", "conflict_out",
                                                  "tab_winner", "tab_util")])
                task_counts = np.zeros((ticks, 3), np.int64)
            if board is not None:
                if board["status"].shape[0] != n:
                    raise ValueError("the task board was set for another number of agents")
                bs = _lib.BoardState(board["Ks"], board["Kt"], p(self.caps),
                                     *[p(board[k]) for k in ("status", "tab_task", "tab_winner", "tab_util",
                                                             "claim_out", "conflict_out")])
                task_counts = np.zeros((ticks, 3), np.int64)
                ch = _lib.Channel(channel[0], channel[1]) if channel is not None else None
                link_counts = np.zeros((ticks, 2), np.int64)
                over = _lib.BoardOverflow()
                entry = _lib.lib().swarm_update_loop_board_moving if board.get("moving") else \
                    _lib.lib().swarm_update_loop_board
                rc = entry(
                    *head, float(radio_radius), float(sense_radius), *tail, ctypes.byref(refused), board["handle"],
                    ctypes.byref(bs), task_counts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(guard),
                    _lib.stream(), ctypes.byref(ch) if ch is not None else None,
                    link_counts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(over))
                self.last_refused_tick = refused.value
                self.last_board_overflow = None if over.kind == _lib.BOARD_FITS else \
                    (BOARD_OVERFLOW_KINDS[over.kind], int(self.perm[over.agent]))
            elif channel is not None:
                ch = _lib.Channel(channel[0], channel[1])
                link_counts = np.zeros((ticks, 2), np.int64)
                rc = _lib.lib().swarm_update_loop_channel(
                    *head, float(radio_radius), float(sense_radius), *tail, ctypes.byref(refused),
                    ctypes.byref(tk) if tk is not None else None,
                    task_counts.ctypes.data_as(ctypes.c_void_p) if tk is not None else None, ctypes.byref(guard),
                    _lib.stream(), ctypes.byref(ch), link_counts.ctypes.data_as(ctypes.c_void_p))
                self.last_refused_tick = refused.value
            elif tasks is not None:
                rc = _lib.lib().swarm_update_loop_tasks(*head, float(radio_radius), float(sense_radius), *tail,
                                                        ctypes.byref(refused), ctypes.byref(tk),
                                                        task_counts.ctypes.data_as(ctypes.c_void_p),
                                                        ctypes.byref(guard), _lib.stream())
                self.last_refused_tick = refused.value
            elif radio_radius is not None:
                rc = _lib.lib().swarm_update_loop_radio(*head, float(radio_radius), float(sense_radius), *tail,
                                                        ctypes.byref(refused), _lib.stream())
                self.last_refused_tick = refused.value
            elif sense_radius is None:
                rc = _lib.lib().swarm_update_loop(
                    *head, _lib.ptr(srp, torch.int32), _lib.ptr(scol, torch.int32) if scol.numel() else None,
                    *tail, _lib.stream())
            else:
                rc = _lib.lib().swarm_update_loop_sensed(*head, float(sense_radius), *tail, ctypes.byref(refused),
                                                         _lib.stream())
                self.last_refused_tick = refused.value
        if n and ticks:
            self._cindex = None  # agents moved: the storage order is no longer their cell order
        self._pos_prev_key = (self.pos, self.pos._version)
        _lib.check(rc)
        self.fsm_tick += ticks
        out = {"counts": counts, "singular": sing.value, "agent_events": agent_events}
        if trace_every:
            out["trace"] = trace
        if tasks is not None or board is not None:
            out["task_counts"], out["guard"] = task_counts, guard.value
        if channel is not None:
            out["link_counts"] = link_counts
        return out

    # ------------------------------------------------------------------ storage order (R1)
    def _resort_arrays(self):
        """Every per-agent array the swarm holds, as (put, tensor, halves): put(new) stores its replacement;
        halves = 2 for the arrays kept by tick parity (2 n rows: both halves take the same permutation)."""
        out = []

        def attr(name, halves=1):
            out.append((lambda t, name=name: setattr(self, name, t), getattr(self, name), halves))

        def item(d, key, halves=1):
            out.append((lambda t, d=d, key=key: d.__setitem__(key, t), d[key], halves))
        for name in ("ids", "pos", "caps", "leader", "state"):
            attr(name)
        if hasattr(self, "vel"):
            for name in ("vel", "target", "has_target"):
                attr(name)
        if hasattr(self, "pos_prev") and self._pos_prev_valid():
            attr("pos_prev")
        if hasattr(self, "tick_off"):
            attr("tick_off")
        if hasattr(self, "fsm"):
            for key in ("last_hb", "wait_start", "delay", "leader_pos", "has_leader_pos", "alive"):
                item(self.fsm, key)
            item(self.fsm, "outbox", 2)
        if hasattr(self, "tasks"):
            for key in ("status_lo", "status_hi", "tab_winner", "tab_util"):
                item(self.tasks, key)
            for key in ("claim_out", "conflict_out"):
                item(self.tasks, key, 2)
        if hasattr(self, "board"):
            for key in ("status", "tab_task", "tab_winner", "tab_util"):
                item(self.board, key)
            for key in ("claim_out", "conflict_out"):
                item(self.board, key, 2)
        return out

    def _pos_prev_valid(self) -> bool:
        """self.pos_prev is one tick behind self.pos (the next loop call would keep it)."""
        k = getattr(self, "_pos_prev_key", None)
        return k is not None and k[0] is self.pos and k[1] == self.pos._version

    def _relabelled(self, frm, row_ptr, col):
        """(row_ptr, col) in the numbering of `frm` (swarm_graph_relabel), as new tensors."""
        rp = torch.empty_like(row_ptr)
        cl = torch.empty_like(col)
        _lib.check(_lib.lib().swarm_graph_relabel(
            _lib.ctx(), self.n, _lib.ptr(frm, torch.int32), _lib.ptr(row_ptr, torch.int32),
            _lib.ptr(col, torch.int32) if col.numel() else None, _lib.ptr(rp), _lib.ptr(cl) if cl.numel() else None,
            _lib.stream()))
        return rp, cl

    def resort(self):
        """Restore the spatial storage order after the agents have moved (contract R1): the swarm
        becomes, array for array and byte for byte, the Swarm one would construct from the input-order view of
        its state.  self.perm is swarm_cell_order of the current positions in input order (agents of a cell by
        input index); every per-agent array -- ids, pos, caps, leader, state, the motion state, a valid pos_prev,
        tick_off, the fsm, the 64-task board's and the task board's arrays, the parity halves of the outboxes
        included -- moves by one row permutation on the device (swarm_permute_rows), so to_input_order of each
        is bit for bit what it was; the neighbour graph names the same neighbours in the same row order in the
        new indices (swarm_graph_relabel; the hearers of a directed graph are its transpose with ascending
        rows, as set_graph builds them).  The election then finds its 16-bit columns again and allocate() its
        cell index.  Tensors are replaced, never overwritten, and only after every device call has gone
        through: a failure leaves the swarm as it was (SwarmError ERR_ARG for a NaN or infinite position).
        Results of earlier calls (ElectResult.leader, AllocResult.won, traces, ...) stay in the storage order
        of their time: self.resorts counts the calls that changed the order, so a holder can tell.
        self.last_resort_moved: the rows whose index changed; 0 (no agent changes index, or n <= 1) rewrites
        nothing and keeps every tensor's identity.  layout="input" raises ValueError: the caller asked for its
        own numbering."""
        if self.layout == "input":
            raise ValueError("resort: the swarm was made with layout='input', which keeps the caller's numbering")
        n, dev = self.n, self.device
        if n <= 1:
            self.last_resort_moved = 0
            return self
        L = _lib.lib()
        frm = torch.empty(n, dtype=torch.int32, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        moved = ctypes.c_int64(0)
        with torch.cuda.device(dev):
            _lib.check(L.swarm_resort_plan(_lib.ctx(), n, _lib.ptr(self.pos, torch.float64),
                                           _lib.ptr(self.perm, torch.int32), self.cell, _lib.ptr(frm), _lib.ptr(perm),
                                           ctypes.byref(moved), _lib.stream()))
            if moved.value == 0:
                self.last_resort_moved = 0
                return self
            arrays = [a for a in self._resort_arrays() if a[1].numel()]
            new, descs = [], []
            for _put, t, halves in arrays:
                if not t.is_contiguous() or t.shape[0] != halves * n:
                    raise ValueError("resort: a per-agent array is not contiguous or was set for another n")
                out = torch.empty_like(t)
                rb = t.element_size() * (t.numel() // (halves * n))
                new.append(out)
                descs += [_lib.Rows(t.data_ptr() + h * n * rb, out.data_ptr() + h * n * rb, rb) for h in range(halves)]
            for lo in range(0, len(descs), 64):
                part = descs[lo:lo + 64]
                _lib.check(L.swarm_permute_rows(_lib.ctx(), n, _lib.ptr(frm), len(part),
                                                (_lib.Rows * len(part))(*part), _lib.stream()))
            graph = hear = None
            if self.row_ptr is not None:
                graph = self._relabelled(frm, self.row_ptr, self.col)
                if getattr(self, "_hear", None) is not None:
                    # the transpose's rows are ascending in set_graph: sorted again in the new indices
                    hrp, hcol = self._relabelled(frm, *self._hear)
                    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev),
                                                   (hrp[1:] - hrp[:-1]).long())
                    hear = (hrp, (torch.sort(rows * n + hcol.long())[0] % n).to(torch.int32))
        pos_prev_kept = hasattr(self, "pos_prev") and self._pos_prev_valid()
        for (put, _t, _h), out in zip(arrays, new):
            put(out)
        self.perm = perm
        if graph is not None:
            self.row_ptr, self.col = graph
            self._hear = hear
        # everything keyed on the old order
        self._c16 = self._rp64 = self._pairs = self._again = self._id_index = None
        self._cindex = self._cindex_key = self._cindex_bad = None
        if pos_prev_kept:
            self._pos_prev_key = (self.pos, self.pos._version)
        else:
            self._pos_prev_key = None
            if hasattr(self, "pos_prev"):
                del self.pos_prev
        self.resorts += 1
        self.last_resort_moved = moved.value
        return self

    # ------------------------------------------------------------------ views / bridge
    def to_input_order(self, storage_tensor) -> np.ndarray:
        """Host copy of a per-agent tensor re-ordered to the caller's input numbering."""
        a = storage_tensor.cpu().numpy()
        out = np.empty_like(a)
        out[self.perm.cpu().numpy()] = a
        return out

    @classmethod
    def from_agents(cls, agents, neighbors=None, cap_vocab=CAP_VOCAB_DEFAULT, device=None, layout="spatial"):
        """Batch a population of agent.SwarmAgent objects (drop-in bridge).

        neighbors: list of neighbour-index lists (who agent i hears), or None to build the
        radius-1 graph from positions on the GPU."""
        if len(cap_vocab) > CAP_UNHELD_BIT:
            raise ValueError(f"at most {CAP_UNHELD_BIT} capability names (bit {CAP_UNHELD_BIT} is reserved for "
                             f"capabilities no agent holds), got {len(cap_vocab)}")
        vocab = {c: k for k, c in enumerate(cap_vocab)}
        ids = np.array([a.agent_id for a in agents], np.int32)
        x = np.array([a.position[0] for a in agents], np.float64)
        y = np.array([a.position[1] for a in agents], np.float64)
        caps = np.zeros(len(agents), np.uint32)
        for i, a in enumerate(agents):
            for c in a.capabilities:
                if c not in vocab:
                    raise ValueError(f"capability {c!r} not in the vocabulary {cap_vocab}")
                caps[i] |= np.uint32(1 << vocab[c])
        sw = cls(ids, x, y, caps, device=device, layout=layout)
        sw.cap_vocab = tuple(cap_vocab)
        if neighbors is None:
            sw.build_graph(1.0)
        else:
            rp = np.zeros(len(agents) + 1, np.int64)
            rp[1:] = np.cumsum([len(nb) for nb in neighbors])
            col = np.array([j for nb in neighbors for j in nb], np.int64)
            sw.set_graph(rp, col)
        return sw

    def write_back_election(self, agents, result: ElectResult):
        """Set leader_id / state on the agent objects as the E2 rounds leave them."""
        from agent import AgentState  # the drop-in scalar module
        lead = self.to_input_order(result.leader)
        st = self.to_input_order(result.state)
        for i, a in enumerate(agents):
            a.leader_id = int(lead[i])
            a.state = AgentState(int(st[i]))

    def tasks_from_dict(self, tasks: dict):
        """(task_ids, tx, ty, treq) arrays from a reference-style task dict."""
        vocab = {c: k for k, c in enumerate(getattr(self, "cap_vocab", CAP_VOCAB_DEFAULT))}
        tid = np.array(list(tasks.keys()), np.int64)
        tx = np.array([tasks[k]["pos"][0] for k in tid], np.float64)
        ty = np.array([tasks[k]["pos"][1] for k in tid], np.float64)
        # a required cap outside the vocabulary blocks every agent: the reserved bit no agent holds
        treq = np.array([vocab.get(tasks[k]["required_cap"], CAP_UNHELD_BIT) if "required_cap" in tasks[k] else -1
                         for k in tid], np.int8)
        return tid, tx, ty, treq

    def write_back_allocation(self, agents, task_ids, res: AllocResult, resolver=None):
        """Statuses every agent holds after full TASK_CONFLICT delivery, and the resolver's
        task_claims table (agent.py:320)."""
        winner = res.winner.cpu().numpy()
        util = res.util.cpu().numpy()
        nmsg = res.nmsg.cpu().numpy()
        nclaim = res.nclaim.cpu().numpy()
        for a in agents:
            for k, tid in enumerate(task_ids):
                task = a.tasks.get(int(tid))
                if task is None:
                    continue
                if nmsg[k] > 0:
                    task["status"] = "ASSIGNED" if a.agent_id == winner[k] else "LOCKED"
                elif nclaim[k] > 0 and a.agent_id == winner[k]:
                    task["status"] = "TENTATIVE"  # lone rejected claim of the incumbent
        if resolver is not None:
            for k, tid in enumerate(task_ids):
                if winner[k] >= 0:
                    resolver.task_claims[int(tid)] = {"winner": int(winner[k]), "utility": float(util[k])}
