// Link prediction of the pretraining stage (ref: models/analysis.py:360-406 `PreEncoder`, :697-744 `PreEncoderPL._common_step`):
// every candidate edge e = (s, d) of a task is scored by the dot product <z[s], z[d]> and trained with BCEWithLogitsLoss against
// its membership in the task's true relation.  The reference gathers both endpoint rows into [E, H] matrices, multiplies, sums,
// compacts candidates and true edges to the batch by boolean masks (a host read each), tests membership by torch.isin over
// Cantor-paired keys and scatters the gradient with two index_add_ launches of float atomics.  Here one call serves every link
// task of the step (staff and voice: different features, different candidates), as a table.
//
// agnn_link_bce_fwd_f32: a group of G lanes (G = 4 .. 64, the power of two covering H / 4 float4 columns; a whole wave at H = 256,
//   several column passes above it) owns one candidate: both rows are read once as float4, the products are summed in a fixed
//   order (per lane over its columns, then a butterfly over the group), the row of the true relation's by-source CSR is scanned
//   for d by the same lanes.  A workgroup owns a tile of 64 candidates; wave 0 then takes one candidate per lane for the BCE and
//   the stores, and the tile's loss sum and five integer counts (alive, tp, fp, fn, tn) go to a partial slot; a second kernel of
//   one workgroup per task adds the slots in a fixed order: two runs give
//   the same bits, and nothing is added atomically.  Candidates with an end outside [0, limit) are not alive: no row is read for
//   them, logit 0, label 0, g 0 — the reference's mask compactions (:712-717) without their host reads.
// agnn_link_bce_bwd_f32: dz[i] = scale (sum_{e: s_e = i} g_e z[d_e] + sum_{e: d_e = i} g_e z[s_e]) as a gather-reduce over the
//   candidate list's two CSRs, one row of dz per group, the coefficient fetched through `perm`: every row is written exactly
//   once (no zero fill, no atomics); a self loop appears in both CSRs and so contributes 2 g_e z[i].
// The table, the lane groups, the ends of an edge, the tile record, the final reduction and the argument checks are peredge.h,
// shared with edgedec.hip; here are the dot product, the membership scan, the BCE and link_row's walk.
#include <cmath>

#include "peredge.h"

using namespace agnn;

namespace {

constexpr int kU = 4;           // list entries a group of the backward keeps in flight

struct LinkFwdDev {
  const float* z;
  int64_t ld_z;
  const int64_t* src;
  const int64_t* dst;
  const int32_t* t_rowptr;
  const int32_t* t_col;
  float* logit;
  uint8_t* label;
  float* g;
  int32_t E, limit, first, pad;
};
struct LinkFwdTable : SegTable<LinkFwdDev> {};
struct LinkFinalTable {         // one workgroup per task: no lookup, no count
  FinalDev t[AGNN_MAX_SEG];
};

struct LinkBwdDev {
  const float* z;
  int64_t ld_z;
  const float* g;
  CsrDev s, d;                  // the candidates by source and by destination
  float* dz;
  int64_t ld_dz;
  int32_t n, E, first, pad;
};
struct LinkBwdTable : SegTable<LinkBwdDev> {};
static_assert(sizeof(LinkFwdTable) + 64 <= 4096 && sizeof(LinkBwdTable) + 64 <= 4096, "the tables travel as kernel arguments");

__global__ __launch_bounds__(256) void k_link_fwd(LinkFwdTable tab, int H4, int lg, uint32_t* __restrict__ part) {
  __shared__ float x_s[kTile];
  __shared__ int flag_s[kTile];
  const int tid = threadIdx.x;
  int task;
  find_segment(tab, task);
  const LinkFwdDev& T = tab.t[task];
  const int first = T.first, tile = static_cast<int>(blockIdx.x) - first;   // read once: the tile record takes it again
  const Lanes L = lanes_of(lg);
  const int G = L.G, lig = L.lig;
  const float* __restrict__ z = T.z;
  // Instruction issue bounds this launch, not memory latency (four candidates in flight per group made it slower): a group only
  // gathers and reduces; what one lane per candidate can do — the BCE, the stores — waits for wave 0, one lane per candidate.
  for (int le = L.grp; le < kTile; le += L.gpb) {         // the same trip count for every lane of the workgroup
    const Ends x = edge_ends(T, static_cast<int64_t>(tile) * kTile + le);
    const int64_t s = x.s, d = x.d;
    const bool in = x.in, alive = x.alive;
    float4 a = agnn::f4_zero();
    int hit = 0;
    if (alive) {
      const float* zs = z + s * T.ld_z;
      const float* zd = z + d * T.ld_z;
      for (int c = lig; c < H4; c += G) {
        const float4 u = *reinterpret_cast<const float4*>(zs + 4 * c);
        const float4 v = *reinterpret_cast<const float4*>(zd + 4 * c);
        a.x = fmaf(u.x, v.x, a.x); a.y = fmaf(u.y, v.y, a.y); a.z = fmaf(u.z, v.z, a.z); a.w = fmaf(u.w, v.w, a.w);
      }
      const int r1 = T.t_rowptr[s + 1];
      const int32_t d32 = static_cast<int32_t>(d);
      for (int j = T.t_rowptr[s] + lig; j < r1; j += G) hit |= (T.t_col[j] == d32) ? 1 : 0;
    }
    const float dot = agnn::group_sum((a.x + a.y) + (a.z + a.w), G);
    hit = agnn::group_or(hit, G);
    if (lig == 0) {
      x_s[le] = dot;
      flag_s[le] = (in ? 1 : 0) | (alive ? 2 : 0) | (hit ? 4 : 0);
    }
  }
  __syncthreads();
  if (tid < kTile) {                                       // wave 0: lane = candidate of the tile
    const int flag = flag_s[tid];
    const bool in = flag & 1, alive = flag & 2, hit = flag & 4;
    const float x = x_s[tid];
    float loss = 0.f, gg = 0.f;
    int code = 0;
    if (alive) {
      const float y = hit ? 1.f : 0.f;
      const float t = expf(-fabsf(x));                     // in (0, 1]
      loss = fmaxf(x, 0.f) - x * y + log1pf(t);
      const float sg = x >= 0.f ? 1.f / (1.f + t) : t / (1.f + t);
      gg = sg - y;
      code = confusion_code(x > 0.f, hit);
    }
    if (in) {
      const int64_t e = static_cast<int64_t>(tile) * kTile + tid;
      T.logit[e] = alive ? x : 0.f;
      T.label[e] = static_cast<uint8_t>((alive && hit) ? 1 : 0);
      T.g[e] = gg;
    }
    tile_record(part, first, tile, loss, code);
  }
}

// one workgroup per task
__global__ __launch_bounds__(256) void k_link_final(LinkFinalTable tab, const uint32_t* __restrict__ part) {
  segment_final(tab.t[blockIdx.x], part);
}

// sum over row i of one CSR of g[perm] z[col], columns 4 c .. 4 c + 3
__device__ __forceinline__ void link_row(const CsrDev csr, int i, const float* __restrict__ g, const float* __restrict__ z, int64_t ld_z, int n,
                                         int E, int c, float4& acc) {
  if (E <= 0) return;                                      // no candidate: g and z may be absent
  const int32_t* __restrict__ rowptr = csr.rowptr;
  const int32_t* __restrict__ col = csr.col;
  const int32_t* __restrict__ perm = csr.perm;
  const int r1 = rowptr[i + 1];
  // kU entries in flight, added in list order as one at a time would be.  The loads are unconditional (an idle slot reads the
  // row's last entry, a skipped one g[0] / row 0, and drops it): a load under a condition becomes a branch with its own wait.
  for (int j0 = rowptr[i]; j0 < r1; j0 += kU) {
    int e[kU], o[kU];
    float ge[kU];
    float4 v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool in = j0 + u < r1;
      const int jc = in ? j0 + u : r1 - 1;
      const int pe = perm[jc], po = col[jc];
      e[u] = in ? pe : -1;
      o[u] = in ? po : -1;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool ok = static_cast<unsigned>(e[u]) < static_cast<unsigned>(E) && static_cast<unsigned>(o[u]) < static_cast<unsigned>(n);
      const float gv = g[ok ? e[u] : 0];
      ge[u] = ok ? gv : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)                           // a coefficient of 0 (candidates that are not alive, among them) adds nothing
      v[u] = *reinterpret_cast<const float4*>(z + static_cast<int64_t>(ge[u] != 0.f ? o[u] : 0) * ld_z + 4 * c);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (ge[u] != 0.f) {
        acc.x = fmaf(ge[u], v[u].x, acc.x); acc.y = fmaf(ge[u], v[u].y, acc.y);
        acc.z = fmaf(ge[u], v[u].z, acc.z); acc.w = fmaf(ge[u], v[u].w, acc.w);
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_link_bwd(LinkBwdTable tab, int H4, int lg, const float* __restrict__ scale) {
  int task;
  find_segment(tab, task);
  const LinkBwdDev& T = tab.t[task];
  const int64_t row = group_row(T, lg);
  if (row >= T.n) return;
  const int i = static_cast<int>(row);
  const Lanes L = lanes_of(lg);
  const float sc = scale[task];
  for (int c = L.lig; c < H4; c += L.G) {                      // H > 256: the row's lists are walked once per column pass
    float4 acc = agnn::f4_zero();
    link_row(T.s, i, T.g, T.z, T.ld_z, T.n, T.E, c, acc);
    link_row(T.d, i, T.g, T.z, T.ld_z, T.n, T.E, c, acc);
    *reinterpret_cast<float4*>(T.dz + row * T.ld_dz + 4 * c) = make_float4(sc * acc.x, sc * acc.y, sc * acc.z, sc * acc.w);
  }
}

int check_fwd_task(const agnn_link_task_t& t, int i, int32_t H) {
  const char* who = "link_bce_fwd";
  if (int rc = check_sizes(who, "task", i, t.E, t.n, t.limit, kTile)) return rc;
  if (!t.loss || !t.inv_cnt || !t.counts) return fail(AGNN_EINVAL, "%s: task %d: loss / inv_cnt / counts is null", who, i);
  if (t.E == 0) return AGNN_OK;
  if (!t.src || !t.dst) return fail(AGNN_EINVAL, "%s: task %d: src / dst is null", who, i);
  if (!t.logit || !t.label || !t.g) return fail(AGNN_EINVAL, "%s: task %d: logit / label / g is null", who, i);
  if (t.limit == 0) return AGNN_OK;                        // no candidate is alive: no row is read
  if (!t.z) return fail(AGNN_EINVAL, "%s: task %d: z is null", who, i);
  if (!t.t_rowptr || !t.t_col) return fail(AGNN_EINVAL, "%s: task %d: t_rowptr / t_col is null", who, i);
  return check_rows(who, "task", i, "z", t.z, t.ld_z, H);
}

}  // namespace

extern "C" size_t agnn_link_bce_workspace_bytes(int32_t n_tasks, const agnn_link_task_t* tasks) {
  if (n_tasks <= 0 || n_tasks > AGNN_MAX_SEG || !tasks) return 0;
  int64_t tiles = 0;
  for (int i = 0; i < n_tasks; ++i) tiles += tiles_of(tasks[i].E, kTile);
  return static_cast<size_t>(tiles) * kPartWords * sizeof(uint32_t);
}

extern "C" int agnn_link_bce_fwd_f32(int32_t n_tasks, const agnn_link_task_t* tasks, int32_t H, void* workspace, size_t workspace_bytes,
                                     agnn_stream_t stream_) {
  const char* who = "link_bce_fwd";
  if (int rc = check_h(who, H)) return rc;
  if (int rc = check_segments(who, "n_tasks", n_tasks)) return rc;
  if (n_tasks == 0) return AGNN_OK;
  if (!tasks) return fail(AGNN_EINVAL, "%s: tasks is null", who);
  LinkFwdTable tab;
  LinkFinalTable fin;
  tab.n = n_tasks;
  tab.pad = 0;
  int64_t tiles = 0;
  for (int i = 0; i < n_tasks; ++i) {
    const agnn_link_task_t& t = tasks[i];
    if (int rc = check_fwd_task(t, i, H)) return rc;
    const int64_t nt = tiles_of(t.E, kTile);
    if (int rc = check_grid(who, "tiles of candidates", tiles + nt)) return rc;
    tab.t[i] = LinkFwdDev{t.z, t.ld_z, t.src, t.dst, t.t_rowptr, t.t_col, t.logit, t.label, t.g, static_cast<int32_t>(t.E),
                          static_cast<int32_t>(t.limit), static_cast<int32_t>(tiles), 0};
    fin.t[i] = FinalDev{t.loss, t.inv_cnt, t.counts, static_cast<int32_t>(tiles), static_cast<int32_t>(nt)};
    tiles += nt;
  }
  const size_t need = static_cast<size_t>(tiles) * kPartWords * sizeof(uint32_t);
  if (tiles > 0) {
    if (int rc = check_workspace(who, workspace, workspace_bytes, need, 4)) return rc;
  }
  hipStream_t s = static_cast<hipStream_t>(stream_);
  uint32_t* part = static_cast<uint32_t*>(workspace);
  if (tiles > 0) {
    hipLaunchKernelGGL(k_link_fwd, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, s, tab, H / 4, agnn::group_log2(H / 4), part);
    if (int rc = check_launch(who)) return rc;
  }
  hipLaunchKernelGGL(k_link_final, dim3(static_cast<unsigned>(n_tasks)), dim3(256), 0, s, fin, part);
  return check_launch("link_bce_fwd (final pass)");
}

extern "C" int agnn_link_bce_bwd_f32(int32_t n_tasks, const agnn_link_bwd_t* tasks, int32_t H, const float* scale, agnn_stream_t stream_) {
  const char* who = "link_bce_bwd";
  if (int rc = check_h(who, H)) return rc;
  if (int rc = check_segments(who, "n_tasks", n_tasks)) return rc;
  if (n_tasks == 0) return AGNN_OK;
  if (!tasks) return fail(AGNN_EINVAL, "%s: tasks is null", who);
  LinkBwdTable tab;
  tab.n = n_tasks;
  tab.pad = 0;
  const int lg = agnn::group_log2(H / 4), gpb = 256 >> lg;
  int64_t blocks = 0;
  for (int i = 0; i < n_tasks; ++i) {
    const agnn_link_bwd_t& t = tasks[i];
    if (t.n < 0 || t.n > INT32_MAX) return fail(AGNN_EINVAL, "%s: task %d: n=%lld must be in [0, 2^31)", who, i, (long long)t.n);
    if (t.E < 0 || t.E > INT32_MAX) return fail(AGNN_EINVAL, "%s: task %d: E=%lld must be in [0, 2^31)", who, i, (long long)t.E);
    const int64_t nb = (t.n + gpb - 1) / gpb;
    if (t.n > 0) {
      if (!t.dz) return fail(AGNN_EINVAL, "%s: task %d: dz is null", who, i);
      if (!t.s_rowptr || !t.d_rowptr) return fail(AGNN_EINVAL, "%s: task %d: s_rowptr / d_rowptr is null", who, i);
      if (int rc = check_rows(who, "task", i, "dz", t.dz, t.ld_dz, H)) return rc;
      if (t.E > 0) {
        if (!t.z || !t.g) return fail(AGNN_EINVAL, "%s: task %d: z / g is null", who, i);
        if (!t.s_col || !t.s_perm || !t.d_col || !t.d_perm) return fail(AGNN_EINVAL, "%s: task %d: a col / perm array is null", who, i);
        if (int rc = check_rows(who, "task", i, "z", t.z, t.ld_z, H)) return rc;
      }
    }
    if (int rc = check_grid(who, "workgroups", blocks + nb)) return rc;
    tab.t[i] = LinkBwdDev{t.z, t.ld_z, t.g, {t.s_rowptr, t.s_col, t.s_perm}, {t.d_rowptr, t.d_col, t.d_perm}, t.dz, t.ld_dz,
                          static_cast<int32_t>(t.n), static_cast<int32_t>(t.E), static_cast<int32_t>(blocks), 0};
    blocks += nb;
  }
  if (blocks == 0) return AGNN_OK;
  if (!scale) return fail(AGNN_EINVAL, "%s: scale is null", who);
  hipLaunchKernelGGL(k_link_bwd, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream_), tab, H / 4, lg, scale);
  return check_launch(who);
}
