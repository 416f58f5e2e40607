// Obstacle fields (contract O1): the host side.  The lists are built by obstacle_cells.h from a host
// copy of the caller's list -- once per field, one host wait, not the hot path -- and uploaded as packed
// (x, y, r) triples; physics.hip's field kernels read them.
#include <cmath>
#include <cstring>
#include <new>

#include "obstacle_cells.h"
#include "swarm_common.h"

namespace swarm {

void free_obstacle_field(swarm_obstacle_field *f) {
    if (!f) return;
    if (f->obs) (void)hipFree(f->obs);
    if (f->cell_off) (void)hipFree(f->cell_off);
    if (f->tri) (void)hipFree(f->tri);
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

}  // namespace
}  // namespace swarm

extern "C" {

int swarm_obstacle_field_create(swarm_ctx *ctx, int64_t m, const double *obstacles, swarm_obstacle_field **out,
                                swarm_obstacle_field_info *info, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    SW_ARG(m >= 0 && m < (int64_t(1) << 31), "m out of range");
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
    swarm_obstacle_field *f = new (std::nothrow) swarm_obstacle_field();
    if (!f) {
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    f->m = m;
    f->g = oc.g;
    if (const int rc = upload_field(f, h_obs, oc, s)) {
        free_obstacle_field(f);
        return rc;
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
