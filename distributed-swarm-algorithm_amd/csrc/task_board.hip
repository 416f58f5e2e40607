// Task boards (contract U1-B): the host side.  The grid and the cell lists are built by task_grid.h
// from a host copy of the caller's board -- once per board, one host wait, not the hot path -- and uploaded as
// a cell-sorted copy of (x, y, treq, index); protocol.hip's board kernels read them.
#include <cmath>
#include <cstring>
#include <new>

#include "swarm_common.h"
#include "task_grid.h"
#include "utility.h"

namespace swarm {

void free_board(swarm_board *b) {
    if (!b) return;
    void *const dev[] = {b->tpos, b->treq, b->cell_off, b->sxy, b->sir, b->verdict};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (b->verdict_host) (void)hipHostFree(b->verdict_host);
    delete b;
}

namespace {

// The rest of swarm_board_create once the lists are built: on any error the caller frees b.
int upload_board(swarm_board *b, const std::vector<double> &h_pos, const std::vector<int8_t> &h_req,
                 const TaskCells &tc, hipStream_t s) {
    const size_t T = size_t(tc.T);
    std::vector<double> sxy;
    std::vector<int32_t> sir;
    try {
        sxy.resize(T * 2);
        sir.resize(T * 2);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %zu cell-sorted tasks", T);
        return SWARM_ERR_OOM;
    }
    for (size_t q = 0; q < T; ++q) {
        const size_t k = size_t(tc.idx[q]);
        sxy[2 * q] = h_pos[2 * k], sxy[2 * q + 1] = h_pos[2 * k + 1];
        sir[2 * q] = int32_t(k), sir[2 * q + 1] = int32_t(h_req[k]);
    }
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->tpos), (T ? T : 1) * 16));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->treq), T ? T : 1));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->cell_off), tc.cell_off.size() * 4));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->sxy), (T ? T : 1) * 16));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->sir), (T ? T : 1) * 8));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->verdict), 64));
    SW_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->verdict_host), 64, hipHostMallocDefault));
    SW_HIP(hipMemcpyAsync(b->cell_off, tc.cell_off.data(), tc.cell_off.size() * 4, hipMemcpyHostToDevice, s));
    if (T) {
        SW_HIP(hipMemcpyAsync(b->tpos, h_pos.data(), T * 16, hipMemcpyHostToDevice, s));
        SW_HIP(hipMemcpyAsync(b->treq, h_req.data(), T, hipMemcpyHostToDevice, s));
        SW_HIP(hipMemcpyAsync(b->sxy, sxy.data(), T * 16, hipMemcpyHostToDevice, s));
        SW_HIP(hipMemcpyAsync(b->sir, sir.data(), T * 8, hipMemcpyHostToDevice, s));
    }
    SW_HIP(hipStreamSynchronize(s));  // the host vectors above end with this call
    return SWARM_OK;
}

swarm_board_desc describe(const swarm_board &b) {
    return swarm_board_desc{b.T, b.g.ncx, b.g.ncy, b.g.cell, b.g.xmin, b.g.ymin, b.longest};
}

}  // namespace
}  // namespace swarm

extern "C" {

int swarm_board_create(swarm_ctx *ctx, int64_t T, const double *tpos, const int8_t *treq, swarm_board **out,
                       swarm_board_desc *info, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && out != nullptr, "ctx or out is NULL");
    SW_ARG(T >= 0 && T <= kMaxBoardTasks, "T must be in [0, 2^24]");
    SW_ARG(T == 0 || (tpos != nullptr && treq != nullptr), "NULL task array");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<double> h_pos;
    std::vector<int8_t> h_req;
    TaskCells tc;
    try {
        h_pos.resize(size_t(T) * 2);
        h_req.resize(size_t(T));
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for a board of %lld tasks", static_cast<long long>(T));
        return SWARM_ERR_OOM;
    }
    if (T) {
        SW_HIP(hipMemcpyAsync(h_pos.data(), tpos, size_t(T) * 16, hipMemcpyDeviceToHost, s));
        SW_HIP(hipMemcpyAsync(h_req.data(), treq, size_t(T), hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    for (int64_t k = 0; k < T; ++k) SW_ARG(!bad_req(h_req[size_t(k)]), "a treq outside [-1, 31]");
    switch (build_task_cells(T, h_pos.data(), &tc)) {
    case kTaskCellsOk:
        break;
    case kTaskCellsNonFinite:
        SW_ARG(false, "task positions must be finite");
    case kTaskCellsExtent:
        set_error("invalid argument: %s", kExtentError);
        return SWARM_ERR_ARG;
    default:
        set_error("out of host memory for the board's cell lists");
        return SWARM_ERR_OOM;
    }
    swarm_board *b = new (std::nothrow) swarm_board();
    if (!b) {
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    b->T = T;
    b->g = tc.g;
    b->longest = tc.longest;
    if (const int rc = upload_board(b, h_pos, h_req, tc, s)) {
        free_board(b);
        return rc;
    }
    b->cell_off_host = std::move(tc.cell_off);
    b->idx_host = std::move(tc.idx);
    try {
        ctx->boards.push_back(b);
    } catch (const std::bad_alloc &) {
        free_board(b);
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    if (info) *info = describe(*b);
    *out = b;
    return SWARM_OK;
}

int swarm_board_info(const swarm_board *board, swarm_board_desc *info) {
    using namespace swarm;
    SW_ARG(board != nullptr && info != nullptr, "board or info is NULL");
    *info = describe(*board);
    return SWARM_OK;
}

int swarm_board_read(const swarm_board *board, uint32_t *cell_off_host, int32_t *idx_host) {
    using namespace swarm;
    SW_ARG(board != nullptr, "board is NULL");
    if (cell_off_host) memcpy(cell_off_host, board->cell_off_host.data(), board->cell_off_host.size() * 4);
    if (idx_host && !board->idx_host.empty()) memcpy(idx_host, board->idx_host.data(), board->idx_host.size() * 4);
    return SWARM_OK;
}

int swarm_board_destroy(swarm_ctx *ctx, swarm_board *board) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    if (!board) return SWARM_OK;
    auto &v = ctx->boards;
    auto it = v.begin();
    while (it != v.end() && *it != board) ++it;
    SW_ARG(it != v.end(), "the board is not a live board of this ctx");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    SW_HIP(hipDeviceSynchronize());  // queued work may still read the board
    v.erase(it);
    free_board(board);
    return SWARM_OK;
}

}  // extern "C"
