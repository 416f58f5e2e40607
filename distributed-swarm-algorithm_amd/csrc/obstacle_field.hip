// Obstacle fields (contract O1): the host side.  The lists are built by obstacle_cells.h from a host
// copy of the caller's list -- once per field, one host wait, not the hot path -- and uploaded as packed
// (x, y, r) triples; physics.hip's field kernels read them.
#include <cmath>
#include <cstring>
#include <new>

#include "binning.h"
#include "fsm_records.h"
#include "obstacle_cells.h"
#include "obstacle_motion.h"
#include "swarm_common.h"

namespace swarm {

void free_obstacle_field(swarm_obstacle_field *f) {
    if (!f) return;
    if (f->obs) (void)hipFree(f->obs);
    if (f->cell_off) (void)hipFree(f->cell_off);
    if (f->tri) (void)hipFree(f->tri);
    void *const more[] = {f->vel, f->entry, f->start, f->keys[0], f->keys[1], f->vals[0], f->vals[1], f->dyn_off,
                          f->dyn_tri, f->cub_tmp, f->err};
    for (void *p : more)
        if (p) (void)hipFree(p);
    delete f;
}

namespace {

// The rest of swarm_obstacle_field_create once the lists are built: on any error the caller frees f.
int upload_field(swarm_obstacle_field *f, const std::vector<double> &h_obs, const ObsCells &oc, hipStream_t s) {
    const size_t m3 = size_t(oc.m) * 3, pairs = size_t(oc.pairs);
    std::vector<double> tri;
    try {
        tri.resize(pairs * 3);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %zu obstacle triples", pairs);
        return SWARM_ERR_OOM;
    }
    for (size_t q = 0; q < pairs; ++q) {
        const double *o = h_obs.data() + size_t(oc.idx[q]) * 3;
        tri[3 * q] = o[0], tri[3 * q + 1] = o[1], tri[3 * q + 2] = o[2];
    }
    // (never a zero-byte allocation: the list's pointer is the field's key, also for m == 0)
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&f->obs), (m3 ? m3 : 2) * 8));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&f->cell_off), oc.cell_off.size() * 4));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&f->tri), (pairs ? pairs * 3 : 2) * 8));
    if (m3) SW_HIP(hipMemcpyAsync(f->obs, h_obs.data(), m3 * 8, hipMemcpyHostToDevice, s));
    SW_HIP(hipMemcpyAsync(f->cell_off, oc.cell_off.data(), oc.cell_off.size() * 4, hipMemcpyHostToDevice, s));
    if (pairs) SW_HIP(hipMemcpyAsync(f->tri, tri.data(), pairs * 24, hipMemcpyHostToDevice, s));
    SW_HIP(hipStreamSynchronize(s));  // the host vectors above end with this call
    return SWARM_OK;
}

// ---- moving fields (contract O2): the cell lists built on the device, every tick ----
//
// The builder is obstacle_cells.h's construction on the device: the same live test, half side and cell range
// per obstacle (k_obs_count / k_obs_emit below are obs_half_side and obs_cell_range, statement for statement,
// with the device's own cell_coord), the pairs emitted obstacle by obstacle at the slice an exclusive sum gives,
// a stable radix sort by cell key -- the pairs of a cell keep their emission order, ascending obstacle index --
// the offsets by search and the triples gathered from the list as it stands.  No atomics: the same lists on
// every run, the host builder's lists on the same grid.

// The footprint's cell range of a live obstacle; false for a dead one.
struct CellRange {
    int64_t x0, x1, y0, y1;
};
__device__ __forceinline__ bool obstacle_range(const double *__restrict__ o, const Grid &g, CellRange *c) {
    const double ox = o[0], oy = o[1], rr = 5.0 + o[2];  // the flat loop's own expression
    if (!(rr > 0)) return false;
    const double h = rr * (1.0 + 1e-9);
    c->x0 = cell_coord(ox - h, g.xmin, g.inv_cell, g.ncx);
    c->x1 = cell_coord(ox + h, g.xmin, g.inv_cell, g.ncx);
    c->y0 = cell_coord(oy - h, g.ymin, g.inv_cell, g.ncy);
    c->y1 = cell_coord(oy + h, g.ymin, g.inv_cell, g.ncy);
    return true;
}

// cnt[o] = the pairs of obstacle o, cnt[m] = 0 (the exclusive sum's last entry is then the total).
__global__ __launch_bounds__(kBlock) void k_obs_count(int64_t m, const double *__restrict__ obs, Grid g,
                                                      unsigned long long *__restrict__ cnt) {
    for (int64_t o = int64_t(blockIdx.x) * kBlock + threadIdx.x; o <= m; o += int64_t(gridDim.x) * kBlock) {
        CellRange c;
        unsigned long long k = 0;
        if (o < m && obstacle_range(obs + 3 * o, g, &c))
            k = (unsigned long long)(c.x1 - c.x0 + 1) * (unsigned long long)(c.y1 - c.y0 + 1);
        cnt[o] = k;
    }
}

// The pairs (cell key, obstacle index) of every obstacle at its slice [start[o], start[o + 1]) of the buffers,
// row by row as the host builder walks a footprint; the tail [total, cap) holds the key `ncells`, past the last
// cell.  total > cap (the capacity bound of obstacle_motion.h failed: never seen, never trusted): nothing but
// that key is written, the error word is set and the run is refused at this tick through its stop word.
// Bounds: a slice is written only when total <= cap, and then start[o + 1] <= total <= cap.
__global__ __launch_bounds__(kBlock) void k_obs_emit(int64_t m, const double *__restrict__ obs, Grid g,
                                                     const unsigned long long *__restrict__ start, int64_t cap,
                                                     uint32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                     unsigned long long *__restrict__ err,
                                                     unsigned long long *__restrict__ st, int32_t k) {
    const unsigned long long total = start[m];
    const uint32_t past = uint32_t(g.ncx * g.ncy);
    const int64_t tid = int64_t(blockIdx.x) * kBlock + threadIdx.x, nth = int64_t(gridDim.x) * kBlock;
    const bool over = total > (unsigned long long)cap;
    for (int64_t q = (over ? 0 : int64_t(total)) + tid; q < cap; q += nth) {
        keys[q] = past;
        vals[q] = 0;
    }
    if (over) {
        if (tid == 0) {
            err[0] = 1;
            if (st[0] == 0) {
                st[2] = 0;
                st[3] = 0;
                st[0] = 1ull + unsigned(k);
            }
        }
        return;
    }
    for (int64_t o = tid; o < m; o += nth) {
        CellRange c;
        if (!obstacle_range(obs + 3 * o, g, &c)) continue;
        unsigned long long q = start[o];
        for (int64_t y = c.y0; y <= c.y1; ++y)
            for (int64_t x = c.x0; x <= c.x1; ++x, ++q) {
                keys[q] = uint32_t(y * g.ncx + x);
                vals[q] = int32_t(o);
            }
    }
}

// The sorted pairs' triples from the list as it stands (a tail pair: nothing).
__global__ __launch_bounds__(kBlock) void k_obs_gather(int64_t cap, uint32_t ncells, int64_t m,
                                                       const uint32_t *__restrict__ skeys,
                                                       const int32_t *__restrict__ svals,
                                                       const double *__restrict__ obs, double *__restrict__ tri) {
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < cap; q += int64_t(gridDim.x) * kBlock) {
        const int64_t o = svals[q];
        if (skeys[q] >= ncells || o < 0 || o >= m) continue;
        tri[3 * q] = obs[3 * o], tri[3 * q + 1] = obs[3 * o + 1], tri[3 * q + 2] = obs[3 * o + 2];
    }
}

// The contract's advance: x <- fl(x + fl(vx * dt)), y likewise (-ffp-contract=off: two roundings), r untouched,
// live and dead obstacles alike.  Nothing once the run's stop word is set.
__global__ __launch_bounds__(kBlock) void k_obs_advance(const unsigned long long *__restrict__ st, int64_t m,
                                                        double *__restrict__ obs, const double *__restrict__ vel,
                                                        double dt) {
    if (st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    for (int64_t o = int64_t(blockIdx.x) * kBlock + threadIdx.x; o < m; o += int64_t(gridDim.x) * kBlock) {
        const double dx = vel[2 * o] * dt, dy = vel[2 * o + 1] * dt;
        obs[3 * o] = obs[3 * o] + dx;
        obs[3 * o + 1] = obs[3 * o + 1] + dy;
    }
}

// The list back to its entry bits when a tick of the loop was refused (protocol.hip's k_restore_refused, for
// the array the field owns).
__global__ __launch_bounds__(kBlock) void k_obs_restore(const unsigned long long *__restrict__ st, int64_t words,
                                                        double *__restrict__ obs, const double *__restrict__ entry) {
    if (st[0] == 0) return;
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < words; q += int64_t(gridDim.x) * kBlock)
        obs[q] = entry[q];
}

int radix_bits(int64_t ncells) {  // keys 0 .. ncells (the tail's key included)
    int b = 1;
    while (b < 32 && (int64_t(1) << b) <= ncells) ++b;
    return b;
}

// p <- a device buffer of at least `bytes` (never zero), *have its size: grown by a new allocation (hipFree
// waits for the device: no queued work reads the old one).
template <typename T>
int grow(T **p, size_t *have, size_t bytes) {
    if (*p && *have >= bytes) return SWARM_OK;
    bytes = bytes < 64 ? 64 : bytes;
    if (*p) SW_HIP(hipFree(*p));
    *p = nullptr, *have = 0;
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("out of device memory for %zu bytes of a moving obstacle field", bytes);
        return SWARM_ERR_OOM;
    }
    *p = static_cast<T *>(q), *have = bytes;
    return SWARM_OK;
}

// The field's buffers for `cap` pairs on a grid of `ncells` cells.
int size_buffers(swarm_obstacle_field *f, int64_t cap, int64_t ncells, hipStream_t s) {
    const size_t pairs = size_t(cap ? cap : 1), cells = size_t(ncells) + 1;
    int rc;
    if (f->cap_pairs < pairs) {
        size_t have[5] = {f->cap_pairs * 4, f->cap_pairs * 4, f->cap_pairs * 4, f->cap_pairs * 4, f->cap_pairs * 24};
        f->cap_pairs = 0;
        if ((rc = grow(&f->keys[0], &have[0], pairs * 4)) || (rc = grow(&f->keys[1], &have[1], pairs * 4)) ||
            (rc = grow(&f->vals[0], &have[2], pairs * 4)) || (rc = grow(&f->vals[1], &have[3], pairs * 4)) ||
            (rc = grow(&f->dyn_tri, &have[4], pairs * 24)))
            return rc;
        f->cap_pairs = pairs;
    }
    if (f->cap_cells < cells) {
        size_t have = f->cap_cells * 4;
        f->cap_cells = 0;
        if ((rc = grow(&f->dyn_off, &have, cells * 4))) return rc;
        f->cap_cells = cells;
    }
    size_t sort_bytes = 0, scan_bytes = 0;
    if (cap)
        SW_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, f->keys[0], f->keys[1], f->vals[0], f->vals[1],
                                                  int(cap), 0, radix_bits(ncells), s));
    SW_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, f->start, f->start, int(f->m + 1), s));
    const size_t tmp = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    return grow(reinterpret_cast<uint8_t **>(&f->cub_tmp), &f->cap_tmp, tmp);
}

// The cell lists of the list as it stands on grid g, queued on s (tick k of a run with stop word st).
int build_lists(swarm_obstacle_field *f, const Grid &g, int64_t cap, unsigned long long *st, int32_t k, hipStream_t s) {
    const int64_t m = f->m, ncells = g.ncx * g.ncy;
    unsigned long long *cnt = f->start, *start = f->start + (m + 1);
    hipLaunchKernelGGL(k_obs_count, dim3(grid_for(m + 1, kBlock, 4096)), dim3(kBlock), 0, s, m, f->obs, g, cnt);
    SW_LAUNCHED();
    size_t tmp = f->cap_tmp;
    SW_HIP(hipcub::DeviceScan::ExclusiveSum(f->cub_tmp, tmp, cnt, start, int(m + 1), s));
    hipLaunchKernelGGL(k_obs_emit, dim3(grid_for(m > cap ? m : cap, kBlock, 4096)), dim3(kBlock), 0, s, m, f->obs, g,
                       start, cap, f->keys[0], f->vals[0], f->err, st, k);
    SW_LAUNCHED();
    if (cap) {
        tmp = f->cap_tmp;
        SW_HIP(hipcub::DeviceRadixSort::SortPairs(f->cub_tmp, tmp, f->keys[0], f->keys[1], f->vals[0], f->vals[1],
                                                  int(cap), 0, radix_bits(ncells), s));
    }
    hipLaunchKernelGGL(k_cell_offsets_search, dim3(grid_for(ncells + 1, kBlock, 8192)), dim3(kBlock), 0, s, f->keys[1],
                       cap, ncells, f->dyn_off);
    SW_LAUNCHED();
    if (cap) {
        hipLaunchKernelGGL(k_obs_gather, dim3(grid_for(cap, kBlock, 8192)), dim3(kBlock), 0, s, cap, uint32_t(ncells), m,
                           f->keys[1], f->vals[1], f->obs, f->dyn_tri);
        SW_LAUNCHED();
    }
    return SWARM_OK;
}

constexpr int64_t kMaxObsCells = int64_t(1) << 31;  // the pairs' cell keys are 32-bit, `ncells` itself is one

int motion_error(ObsMotionStatus st) {
    switch (st) {
    case kObsMotionOk:
        return SWARM_OK;
    case kObsMotionNonFinite:
        set_error("invalid argument: an obstacle entry or velocity is not finite");
        return SWARM_ERR_ARG;
    case kObsMotionExtent:
        set_error("invalid argument: the moving obstacles' footprints have no finite extent over the call");
        return SWARM_ERR_ARG;
    default:
        set_error("the moving obstacle field may need more than %lld (cell, obstacle) pairs on this grid (the bound "
                  "from the radii): obstacles that reach very many 10-unit cells",
                  static_cast<long long>(kMaxObsPairs));
        return SWARM_ERR_RANGE;
    }
}

int check_cells(const Grid &g) {
    if (g.ncx * g.ncy <= kMaxObsCells) return SWARM_OK;
    set_error("a moving obstacle field's grid is limited to 2^31 cells");
    return SWARM_ERR_RANGE;
}

// The device velocities (NULL: zero) to the host, refused unless finite.
int fetch_velocities(int64_t m, const double *velocities, std::vector<double> *out, hipStream_t s) {
    try {
        out->assign(size_t(m) * 2, 0.0);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %lld velocities", static_cast<long long>(m));
        return SWARM_ERR_OOM;
    }
    if (m && velocities) {
        SW_HIP(hipMemcpyAsync(out->data(), velocities, size_t(m) * 16, hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    SW_ARG(obs_velocities_finite(m, out->data()), "a velocity is not finite");
    return SWARM_OK;
}

bool live_field(const swarm_ctx *ctx, const swarm_obstacle_field *field) {
    for (const swarm_obstacle_field *f : ctx->fields)
        if (f == field) return true;
    return false;
}

}  // namespace

swarm_obstacle_field *find_moving_field(swarm_ctx *ctx, int64_t m, const double *obstacles) {
    if (obstacles)
        for (swarm_obstacle_field *f : ctx->fields)
            if (f->obs == obstacles && f->m == m) return f->moving ? f : nullptr;
    return nullptr;
}

int moving_field_fetch(swarm_obstacle_field *f, hipStream_t s) {
    try {
        f->list_host.resize(size_t(f->m) * 3);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %lld obstacles", static_cast<long long>(f->m));
        return SWARM_ERR_OOM;
    }
    if (f->m) SW_HIP(hipMemcpyAsync(f->list_host.data(), f->obs, size_t(f->m) * 24, hipMemcpyDeviceToHost, s));
    return SWARM_OK;
}

int moving_field_begin(swarm_obstacle_field *f, int32_t ticks, double dt, bool keep_entry, hipStream_t s) {
    ObsCallPlan plan;
    int rc;
    if ((rc = motion_error(plan_obstacle_call(f->m, f->list_host.data(), f->vel_host.data(), dt, ticks, &plan))))
        return rc;
    if ((rc = check_cells(plan.g))) return rc;
    if ((rc = size_buffers(f, plan.capacity, plan.g.ncx * plan.g.ncy, s))) return rc;
    f->call_g = plan.g;
    f->capacity = plan.capacity;
    SW_HIP(hipMemsetAsync(f->err, 0, 8, s));
    if (keep_entry && f->m)
        SW_HIP(hipMemcpyAsync(f->entry, f->obs, size_t(f->m) * 24, hipMemcpyDeviceToDevice, s));
    return SWARM_OK;
}

int moving_field_tick(swarm_obstacle_field *f, unsigned long long *st, int32_t k, ObsFieldView *view, hipStream_t s) {
    const Grid &g = f->call_g;
    *view = ObsFieldView{f->dyn_off, f->dyn_tri, g.xmin, g.ymin, g.inv_cell, g.ncx, g.ncy};
    return build_lists(f, g, f->capacity, st, k, s);
}

int moving_field_advance(swarm_obstacle_field *f, const unsigned long long *st, double dt, hipStream_t s) {
    if (f->m == 0) return SWARM_OK;
    hipLaunchKernelGGL(k_obs_advance, dim3(grid_for(f->m, kBlock, 4096)), dim3(kBlock), 0, s, st, f->m, f->obs, f->vel,
                       dt);
    SW_LAUNCHED();
    return SWARM_OK;
}

int moving_field_restore_if_refused(swarm_obstacle_field *f, const unsigned long long *st, hipStream_t s) {
    if (f->m == 0) return SWARM_OK;
    hipLaunchKernelGGL(k_obs_restore, dim3(grid_for(f->m * 3, kBlock, 4096)), dim3(kBlock), 0, s, st, f->m * 3, f->obs,
                       f->entry);
    SW_LAUNCHED();
    return SWARM_OK;
}

int moving_field_error(swarm_obstacle_field *f, unsigned long long *h_word, hipStream_t s) {
    SW_HIP(hipMemcpyAsync(h_word, f->err, 8, hipMemcpyDeviceToHost, s));
    return SWARM_OK;
}

int moving_field_overflowed() {
    set_error("a tick's (cell, obstacle) pairs exceeded the moving obstacle field's capacity bound (nothing of the "
              "tick was computed): please report the obstacle list");
    return SWARM_ERR_RANGE;
}

}  // namespace swarm

// swarm_obstacle_field_create (moving false) and swarm_obstacle_field_create_moving.
static int create_field(swarm_ctx *ctx, int64_t m, const double *obstacles, bool moving, const double *velocities,
                        swarm_obstacle_field **out, swarm_obstacle_field_info *info, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    SW_ARG(m >= 0 && m < (int64_t(1) << 31) - (moving ? 1 : 0), "m out of range");  // (moving: m + 1 counts are summed)
    SW_ARG(m == 0 || obstacles != nullptr, "obstacles is NULL");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<double> h_obs;
    ObsCells oc;
    try {
        h_obs.resize(size_t(m) * 3);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %lld obstacles", static_cast<long long>(m));
        return SWARM_ERR_OOM;
    }
    if (m) {
        SW_HIP(hipMemcpyAsync(h_obs.data(), obstacles, size_t(m) * 24, hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    switch (build_obstacle_cells(m, h_obs.data(), &oc)) {
    case kObsCellsOk:
        break;
    case kObsCellsNonFinite:
        set_error("invalid argument: an obstacle entry is not finite");
        return SWARM_ERR_ARG;
    case kObsCellsExtent:
        set_error("invalid argument: the obstacles' footprints have no finite extent (max - min overflows a double)");
        return SWARM_ERR_ARG;
    case kObsCellsPairs:
        set_error("the obstacle field needs more than %lld (cell, obstacle) pairs: obstacles that reach very many "
                  "10-unit cells (pass such a list as a flat list)",
                  static_cast<long long>(kMaxObsPairs));
        return SWARM_ERR_RANGE;
    default:
        set_error("out of host memory for the obstacle field's lists");
        return SWARM_ERR_OOM;
    }
    std::vector<double> h_vel;
    int64_t cap = 0;
    if (moving) {  // its own refusals, before anything is created: the velocities, the capacity on this grid
        int rc;
        if ((rc = fetch_velocities(m, velocities, &h_vel, s))) return rc;
        if ((rc = motion_error(obs_pair_capacity(m, h_obs.data(), oc.g, &cap)))) return rc;
        if ((rc = check_cells(oc.g))) return rc;
    }
    swarm_obstacle_field *f = new (std::nothrow) swarm_obstacle_field();
    if (!f) {
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    f->m = m;
    f->g = oc.g;
    f->live = oc.live;
    if (const int rc = upload_field(f, h_obs, oc, s)) {
        free_obstacle_field(f);
        return rc;
    }
    if (moving) {
        auto extras = [&]() -> int {
            const size_t um = size_t(m);
            SW_HIP(hipMalloc(reinterpret_cast<void **>(&f->vel), (um ? um * 2 : 2) * 8));
            SW_HIP(hipMalloc(reinterpret_cast<void **>(&f->entry), (um ? um * 3 : 2) * 8));
            SW_HIP(hipMalloc(reinterpret_cast<void **>(&f->start), (um + 1) * 2 * 8));
            SW_HIP(hipMalloc(reinterpret_cast<void **>(&f->err), 64));
            SW_HIP(hipMemsetAsync(f->err, 0, 64, s));
            if (um) SW_HIP(hipMemcpyAsync(f->vel, h_vel.data(), um * 16, hipMemcpyHostToDevice, s));
            SW_HIP(hipStreamSynchronize(s));
            return size_buffers(f, cap, oc.g.ncx * oc.g.ncy, s);
        };
        if (const int rc = extras()) {
            free_obstacle_field(f);
            return rc;
        }
        f->moving = true;
        f->vel_host = std::move(h_vel);
        f->call_g = oc.g;
        f->capacity = cap;
    }
    if (info)
        *info = swarm_obstacle_field_info{m, oc.live, oc.g.ncx, oc.g.ncy, oc.g.cell, oc.g.xmin, oc.g.ymin, oc.pairs,
                                          oc.longest};
    f->cell_off_host = std::move(oc.cell_off);
    f->idx_host = std::move(oc.idx);
    try {
        ctx->fields.push_back(f);
    } catch (const std::bad_alloc &) {
        free_obstacle_field(f);
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    *out = f;
    return SWARM_OK;
}

extern "C" {

int swarm_obstacle_field_create(swarm_ctx *ctx, int64_t m, const double *obstacles, swarm_obstacle_field **out,
                                swarm_obstacle_field_info *info, void *stream) {
    return create_field(ctx, m, obstacles, false, nullptr, out, info, stream);
}

int swarm_obstacle_field_create_moving(swarm_ctx *ctx, int64_t m, const double *obstacles, const double *velocities,
                                       swarm_obstacle_field **out, swarm_obstacle_field_info *info, void *stream) {
    return create_field(ctx, m, obstacles, true, velocities, out, info, stream);
}

int swarm_obstacle_field_set_velocities(swarm_ctx *ctx, swarm_obstacle_field *field, const double *velocities,
                                        void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && field != nullptr, "ctx or field is NULL");
    SW_ARG(live_field(ctx, field), "the field is not a live field of this ctx");
    SW_ARG(field->moving, "the field does not move (swarm_obstacle_field_create_moving makes one that does)");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<double> h_vel;
    if (const int rc = fetch_velocities(field->m, velocities, &h_vel, s)) return rc;
    if (field->m) {
        SW_HIP(hipMemcpyAsync(field->vel, h_vel.data(), size_t(field->m) * 16, hipMemcpyHostToDevice, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    field->vel_host = std::move(h_vel);
    return SWARM_OK;
}

int swarm_obstacle_field_refresh(swarm_ctx *ctx, swarm_obstacle_field *field, swarm_obstacle_field_info *info,
                                 void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && field != nullptr, "ctx or field is NULL");
    SW_ARG(live_field(ctx, field), "the field is not a live field of this ctx");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    swarm_obstacle_field *f = field;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t m = f->m;
    int rc;
    if (f->moving) {
        if ((rc = moving_field_fetch(f, s))) return rc;
        SW_HIP(hipStreamSynchronize(s));
        Grid g{};
        int64_t live = 0, cap = 0;
        if ((rc = motion_error(obs_static_grid(m, f->list_host.data(), &g, &live)))) return rc;
        if ((rc = motion_error(obs_pair_capacity(m, f->list_host.data(), g, &cap)))) return rc;
        if ((rc = check_cells(g))) return rc;
        const int64_t ncells = g.ncx * g.ncy;
        if ((rc = size_buffers(f, cap, ncells, s))) return rc;
        unsigned long long *st;  // a stop word of its own: a refresh is no tick of a run
        SW_ALLOC(st, ctx, S_TMP0, 64);
        SW_HIP(hipMemsetAsync(st, 0, 32, s));
        SW_HIP(hipMemsetAsync(f->err, 0, 8, s));
        if ((rc = build_lists(f, g, cap, st, 0, s))) return rc;
        std::vector<uint32_t> off;
        std::vector<int32_t> idx;
        unsigned long long over = 0;
        try {
            off.resize(size_t(ncells) + 1);
            SW_HIP(hipMemcpyAsync(off.data(), f->dyn_off, off.size() * 4, hipMemcpyDeviceToHost, s));
            SW_HIP(hipMemcpyAsync(&over, f->err, 8, hipMemcpyDeviceToHost, s));
            SW_HIP(hipStreamSynchronize(s));
            if (over) return moving_field_overflowed();
            idx.resize(off.back());
            if (!idx.empty()) {
                SW_HIP(hipMemcpyAsync(idx.data(), f->vals[1], idx.size() * 4, hipMemcpyDeviceToHost, s));
                SW_HIP(hipStreamSynchronize(s));
            }
        } catch (const std::bad_alloc &) {
            set_error("out of host memory for the obstacle field's lists");
            return SWARM_ERR_OOM;
        }
        f->g = g;
        f->cell_off_host = std::move(off);
        f->idx_host = std::move(idx);
        f->live = live;
    }
    if (info) {
        int64_t longest = 0;
        const std::vector<uint32_t> &off = f->cell_off_host;
        for (size_t c = 0; c + 1 < off.size(); ++c)
            longest = int64_t(off[c + 1] - off[c]) > longest ? int64_t(off[c + 1] - off[c]) : longest;
        *info = swarm_obstacle_field_info{m, f->live, f->g.ncx, f->g.ncy, f->g.cell, f->g.xmin, f->g.ymin,
                                          int64_t(off.back()), longest};
    }
    return SWARM_OK;
}

int swarm_obstacle_field_obstacles(const swarm_obstacle_field *field, const double **obstacles) {
    using namespace swarm;
    SW_ARG(field != nullptr && obstacles != nullptr, "field or obstacles is NULL");
    *obstacles = field->obs;
    return SWARM_OK;
}

int swarm_obstacle_field_read(const swarm_obstacle_field *field, uint32_t *cell_off_host, int32_t *idx_host) {
    using namespace swarm;
    SW_ARG(field != nullptr, "field is NULL");
    if (cell_off_host) memcpy(cell_off_host, field->cell_off_host.data(), field->cell_off_host.size() * 4);
    if (idx_host && !field->idx_host.empty()) memcpy(idx_host, field->idx_host.data(), field->idx_host.size() * 4);
    return SWARM_OK;
}

int swarm_obstacle_field_destroy(swarm_ctx *ctx, swarm_obstacle_field *field) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    if (!field) return SWARM_OK;
    auto &v = ctx->fields;
    auto it = v.begin();
    while (it != v.end() && *it != field) ++it;
    SW_ARG(it != v.end(), "the field is not a live field of this ctx");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    SW_HIP(hipDeviceSynchronize());  // queued work may still read the field
    v.erase(it);
    free_obstacle_field(field);
    return SWARM_OK;
}

}  // extern "C"
