// KV fork: the first n_rows cache rows of one slot copied to many slots, every plane of a handle in ONE launch (td_kv_fork_rows).
//
// What it is for: n / best_of parallel sampling prefills a prompt once and lets k sequences continue from the same cache rows.  The slots of the
// Qwen2 engine are a fixed partition of each layer's cache, so a fork is a copy.  td_qwen2_move_slot does that copy for ONE destination with one
// hipMemcpyAsync per plane: 28 layers x 2 planes x 7 destinations = 392 host-enqueued copies for an e4m3 prompt forked seven ways, and the source
// rows are read seven times.  Here every source chunk is loaded once and stored n_dst times.
//
// A plane is `slots x slot_rows` rows of row_bytes bytes; the rows [0, n_rows) of a slot are contiguous, so per plane the fork is one byte range of
// n_rows x row_bytes bytes at `base + slot x slot_rows x row_bytes`.  Source and destinations differ by multiples of the slot stride, so they share
// their alignment modulo w = the largest of 16, 8, 4, 2 that divides the stride: with that width ONE split of the range into
//   head  (2-byte pieces up to the first w-aligned address: at most 7),  body (w-byte pieces, w-aligned on every side),  tail (2-byte pieces, at most 7)
// holds for the source and for every destination.  w = 16 whenever the slot stride is a multiple of 16 -- every Qwen2 cache plane but the e4m3 scale
// plane of a one-kv-head model with an odd slot_len (2 Hkv 4 = 8 bytes per row), which is copied in 8-byte pieces.
//
// The plane table and the destination slots travel in the launch's own arguments (td_logit_edits_set_bias's method): nothing is allocated, nothing
// uploaded, no host buffer has to outlive the call; FORK_PLANES planes x FORK_DSTS destinations per launch, as many launches as that needs.
//
// Below the fork: the KV gather (td_kv_gather_rows), the same copy with one source per ROW, named by the device -- the reordering of cache slots
// behind a beam-search step (csrc/beam_search.hip).
#include <algorithm>
#include <vector>

#include "td_common.h"
#include "../../include/thinkdiff_hip.h"

namespace {

constexpr int FORK_PLANES = 64;      // (28 layers x 2 planes of the e4m3 cache fit one launch)
constexpr int FORK_DSTS = 192;
constexpr int FORK_NT = 256;
constexpr int FORK_UNROLL = 4;       // pieces a thread has in flight: 4 x 16 bytes x 256 threads = 16 KiB of source per workgroup and pass

struct ForkPlane {
  char* base;                // the plane
  long long slot_bytes;      // slot stride
  long long nbytes;          // bytes to copy per slot
  int w;                     // access width of the body: 16, 8, 4 or 2
  int head;                  // bytes before the first w-aligned address (even, < w, <= nbytes)
};
struct ForkArgs {            // 64 x 32 + 192 x 4 + 16 = 2832 bytes of kernel arguments
  ForkPlane plane[FORK_PLANES];
  int dst[FORK_DSTS];
  int src;
  int n_dst;
  int pad0, pad1;
};

template <typename T>
__device__ __forceinline__ void fork_body(const ForkArgs& a, const ForkPlane& p, long long pieces) {
  const char* src = p.base + (long long)a.src * p.slot_bytes + p.head;
  const long long per_pass = (long long)FORK_NT * FORK_UNROLL;
  for (long long c0 = (long long)blockIdx.x * per_pass; c0 < pieces; c0 += (long long)gridDim.x * per_pass) {
    T v[FORK_UNROLL];
#pragma unroll
    for (int u = 0; u < FORK_UNROLL; ++u) {
      const long long c = c0 + u * FORK_NT + threadIdx.x;
      if (c < pieces) v[u] = ((const T*)src)[c];
    }
    for (int d = 0; d < a.n_dst; ++d) {
      char* dst = p.base + (long long)a.dst[d] * p.slot_bytes + p.head;
#pragma unroll
      for (int u = 0; u < FORK_UNROLL; ++u) {
        const long long c = c0 + u * FORK_NT + threadIdx.x;
        if (c < pieces) ((T*)dst)[c] = v[u];
      }
    }
  }
}

// grid (passes, planes of this launch): workgroup x of plane y walks the body's pieces x, x + gridDim.x, ..; workgroup 0 of a plane also copies the
// head (threads 0 ..) and the tail (threads 64 ..) in 2-byte pieces
__global__ __launch_bounds__(FORK_NT) void td_kv_fork_kernel(const ForkArgs a) {
  const ForkPlane& p = a.plane[blockIdx.y];
  const long long body = (p.nbytes - p.head) / p.w;
  if (blockIdx.x == 0) {
    const int tail = (int)(p.nbytes - p.head - body * p.w);
    const int t = threadIdx.x;
    long long off = -1;
    if (t < p.head / 2) off = 2 * t;
    else if (t >= 64 && t - 64 < tail / 2) off = p.head + body * p.w + 2 * (t - 64);
    if (off >= 0) {
      const unsigned short v = *(const unsigned short*)(p.base + (long long)a.src * p.slot_bytes + off);
      for (int d = 0; d < a.n_dst; ++d) *(unsigned short*)(p.base + (long long)a.dst[d] * p.slot_bytes + off) = v;
    }
  }
  if (p.w == 16) fork_body<u32x4_t>(a, p, body);
  else if (p.w == 8) fork_body<u32x2_t>(a, p, body);
  else if (p.w == 4) fork_body<unsigned>(a, p, body);
  else fork_body<unsigned short>(a, p, body);
}

// ---- KV gather (td_kv_gather_rows): row j of a launch takes the cache rows of row copy_src[j], which the DEVICE names -------------------------
// Beam search reorders cache slots by what td_beam_select chose, and the host does not know the choice: the slot of every row and its length are
// host values in the launch arguments (the fork's method), the source row is read from device memory.  The split of a byte range into head, body
// and tail is the fork's -- every slot of a plane shares its alignment modulo w -- but the range's length differs per row, so it is made here.
constexpr int GATHER_ROWS = 64;         // destination rows per launch (grid z)
constexpr int GATHER_MAX_N = 256;       // rows of a call: every launch carries the whole slot table, a source may be any row
constexpr int GATHER_PASSES = 32;       // workgroups per (plane, row): a row that copies nothing costs 32 x planes workgroups that return at once

struct GatherPlane {
  char* base;
  long long slot_bytes;
  int row_bytes;
  int w;                     // access width of the body
};
struct GatherArgs {          // 64 x 24 + 256 x 4 + 64 x 4 + 16 = 2832 bytes of kernel arguments
  GatherPlane plane[FORK_PLANES];
  int slot[GATHER_MAX_N];
  int n_rows[GATHER_ROWS];   // of the rows row0 .. row0 + GATHER_ROWS
  int row0;
  int n;
  int pad0, pad1;
};

template <typename T>
__device__ __forceinline__ void gather_body(const char* src, char* dst, long long pieces) {
  const long long per_pass = (long long)FORK_NT * FORK_UNROLL;
  for (long long c0 = (long long)blockIdx.x * per_pass; c0 < pieces; c0 += (long long)gridDim.x * per_pass) {
    T v[FORK_UNROLL];
#pragma unroll
    for (int u = 0; u < FORK_UNROLL; ++u) {
      const long long c = c0 + u * FORK_NT + threadIdx.x;
      if (c < pieces) v[u] = ((const T*)src)[c];
    }
#pragma unroll
    for (int u = 0; u < FORK_UNROLL; ++u) {
      const long long c = c0 + u * FORK_NT + threadIdx.x;
      if (c < pieces) ((T*)dst)[c] = v[u];
    }
  }
}

// grid (passes, planes of this launch, rows of this launch); a workgroup whose row copies nothing returns before it touches a plane
__global__ __launch_bounds__(FORK_NT) void td_kv_gather_kernel(const GatherArgs a, const int* __restrict__ copy_src) {
  const int j = a.row0 + blockIdx.z;
  const int s = copy_src[j];
  if (s < 0 || s >= a.n || s == j) return;      // (a source outside the call's rows names no slot: nothing is read through it)
  const GatherPlane& p = a.plane[blockIdx.y];
  const long long nbytes = (long long)a.n_rows[blockIdx.z] * p.row_bytes;
  if (nbytes <= 0) return;
  const char* src = p.base + (long long)a.slot[s] * p.slot_bytes;
  char* dst = p.base + (long long)a.slot[j] * p.slot_bytes;
  const int mis = (int)((uintptr_t)src % (uintptr_t)p.w);
  const long long head = min((long long)((p.w - mis) % p.w), nbytes);
  const long long body = (nbytes - head) / p.w;
  if (blockIdx.x == 0) {
    const int tail = (int)(nbytes - head - body * p.w);
    const int t = threadIdx.x;
    long long off = -1;
    if (t < head / 2) off = 2 * t;
    else if (t >= 64 && t - 64 < tail / 2) off = head + body * p.w + 2 * (t - 64);
    if (off >= 0) *(unsigned short*)(dst + off) = *(const unsigned short*)(src + off);
  }
  if (p.w == 16) gather_body<u32x4_t>(src + head, dst + head, body);
  else if (p.w == 8) gather_body<u32x2_t>(src + head, dst + head, body);
  else if (p.w == 4) gather_body<unsigned>(src + head, dst + head, body);
  else gather_body<unsigned short>(src + head, dst + head, body);
}

}  // namespace

extern "C" {

int td_kv_gather_rows(const TdKvPlane* planes, int n_planes, int n, const int* slots, const int32_t* copy_src_dev, const int* n_rows, void* stream) {
  TD_CHECK_ARG(planes, "td_kv_gather_rows: null planes");
  TD_CHECK_ARG(slots, "td_kv_gather_rows: null slots");
  TD_CHECK_ARG(copy_src_dev, "td_kv_gather_rows: null copy_src_dev");
  TD_CHECK_ARG(n_rows, "td_kv_gather_rows: null n_rows");
  TD_CHECK_ARG(n_planes >= 1, "td_kv_gather_rows: n_planes=%d, at least one plane is needed", n_planes);
  TD_CHECK_ARG(n >= 1 && n <= GATHER_MAX_N, "td_kv_gather_rows: n=%d rows outside 1..%d", n, GATHER_MAX_N);
  int max_rows = 0;
  for (int j = 0; j < n; ++j) {
    TD_CHECK_ARG(slots[j] >= 0, "td_kv_gather_rows: slot %d of row %d is negative", slots[j], j);
    TD_CHECK_ARG(n_rows[j] >= 0, "td_kv_gather_rows: n_rows=%d of row %d is negative", n_rows[j], j);
    max_rows = std::max(max_rows, n_rows[j]);
  }
  for (int p = 0; p < n_planes; ++p) {
    TD_CHECK_ARG(planes[p].base, "td_kv_gather_rows: plane %d has a null base", p);
    TD_CHECK_ARG(planes[p].row_bytes >= 2 && planes[p].row_bytes % 2 == 0 && planes[p].row_bytes <= (1 << 30),
                 "td_kv_gather_rows: row_bytes=%lld of plane %d is not a positive multiple of 2", (long long)planes[p].row_bytes, p);
    TD_CHECK_ARG(((uintptr_t)planes[p].base) % 2 == 0, "td_kv_gather_rows: the base %p of plane %d is not 2-byte aligned", planes[p].base, p);
    TD_CHECK_ARG(planes[p].slot_rows >= 1, "td_kv_gather_rows: slot_rows=%lld of plane %d is not positive", (long long)planes[p].slot_rows, p);
    TD_CHECK_ARG(max_rows <= planes[p].slot_rows, "td_kv_gather_rows: n_rows=%d exceeds slot_rows=%lld of plane %d", max_rows, (long long)planes[p].slot_rows, p);
  }
  std::vector<int> sorted(slots, slots + n);
  std::sort(sorted.begin(), sorted.end());
  for (int i = 1; i < n; ++i) TD_CHECK_ARG(sorted[i] != sorted[i - 1], "td_kv_gather_rows: slot %d is given twice", sorted[i]);
  if (max_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  for (int p0 = 0; p0 < n_planes; p0 += FORK_PLANES) {
    const int np = std::min(FORK_PLANES, n_planes - p0);
    GatherArgs a = {};
    a.n = n;
    for (int j = 0; j < n; ++j) a.slot[j] = slots[j];
    for (int p = 0; p < np; ++p) {
      const TdKvPlane& q = planes[p0 + p];
      GatherPlane& gp = a.plane[p];
      gp.base = (char*)q.base;
      gp.slot_bytes = (long long)q.slot_rows * q.row_bytes;
      gp.row_bytes = (int)q.row_bytes;
      gp.w = gp.slot_bytes % 16 == 0 ? 16 : gp.slot_bytes % 8 == 0 ? 8 : gp.slot_bytes % 4 == 0 ? 4 : 2;
    }
    for (int r0 = 0; r0 < n; r0 += GATHER_ROWS) {
      const int nr = std::min(GATHER_ROWS, n - r0);
      a.row0 = r0;
      long long passes = 1;
      for (int j = 0; j < nr; ++j) {
        a.n_rows[j] = n_rows[r0 + j];
        for (int p = 0; p < np; ++p) {
          const long long per_pass = (long long)FORK_NT * FORK_UNROLL * a.plane[p].w;
          passes = std::max(passes, ((long long)n_rows[r0 + j] * a.plane[p].row_bytes + per_pass - 1) / per_pass);
        }
      }
      hipLaunchKernelGGL(td_kv_gather_kernel, dim3((unsigned)std::min<long long>(passes, GATHER_PASSES), np, nr), dim3(FORK_NT), 0, st, a, copy_src_dev);
      TD_CHECK_LAUNCH();
    }
  }
  return 0;
}

int td_kv_fork_rows(const TdKvPlane* planes, int n_planes, int src_slot, const int* dst_slots, int n_dst, int n_rows, void* stream) {
  TD_CHECK_ARG(planes, "td_kv_fork_rows: null planes");
  TD_CHECK_ARG(dst_slots, "td_kv_fork_rows: null dst_slots");
  TD_CHECK_ARG(n_planes >= 1, "td_kv_fork_rows: n_planes=%d, at least one plane is needed", n_planes);
  TD_CHECK_ARG(n_dst >= 1, "td_kv_fork_rows: n_dst=%d, at least one destination is needed", n_dst);
  TD_CHECK_ARG(n_rows >= 0, "td_kv_fork_rows: n_rows=%d is negative", n_rows);
  TD_CHECK_ARG(src_slot >= 0, "td_kv_fork_rows: src_slot=%d is negative", src_slot);
  for (int p = 0; p < n_planes; ++p) {
    TD_CHECK_ARG(planes[p].base, "td_kv_fork_rows: plane %d has a null base", p);
    TD_CHECK_ARG(planes[p].row_bytes >= 2 && planes[p].row_bytes % 2 == 0, "td_kv_fork_rows: row_bytes=%lld of plane %d is not a positive multiple of 2",
                 (long long)planes[p].row_bytes, p);
    TD_CHECK_ARG(((uintptr_t)planes[p].base) % 2 == 0, "td_kv_fork_rows: the base %p of plane %d is not 2-byte aligned", planes[p].base, p);
    TD_CHECK_ARG(planes[p].slot_rows >= 1, "td_kv_fork_rows: slot_rows=%lld of plane %d is not positive", (long long)planes[p].slot_rows, p);
    TD_CHECK_ARG(n_rows <= planes[p].slot_rows, "td_kv_fork_rows: n_rows=%d exceeds slot_rows=%lld of plane %d", n_rows, (long long)planes[p].slot_rows, p);
  }
  std::vector<int> sorted(dst_slots, dst_slots + n_dst);
  std::sort(sorted.begin(), sorted.end());
  TD_CHECK_ARG(sorted[0] >= 0, "td_kv_fork_rows: destination slot %d is negative", sorted[0]);
  for (int i = 0; i < n_dst; ++i) {
    TD_CHECK_ARG(sorted[i] != src_slot, "td_kv_fork_rows: src_slot=%d is among the destinations", src_slot);
    TD_CHECK_ARG(i == 0 || sorted[i] != sorted[i - 1], "td_kv_fork_rows: destination slot %d is given twice", sorted[i]);
  }
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  for (int p0 = 0; p0 < n_planes; p0 += FORK_PLANES) {
    const int np = std::min(FORK_PLANES, n_planes - p0);
    ForkArgs a = {};
    a.src = src_slot;
    long long passes = 1;
    for (int p = 0; p < np; ++p) {
      const TdKvPlane& q = planes[p0 + p];
      ForkPlane& fp = a.plane[p];
      fp.base = (char*)q.base;
      fp.slot_bytes = (long long)q.slot_rows * q.row_bytes;
      fp.nbytes = (long long)n_rows * q.row_bytes;
      fp.w = fp.slot_bytes % 16 == 0 ? 16 : fp.slot_bytes % 8 == 0 ? 8 : fp.slot_bytes % 4 == 0 ? 4 : 2;
      const long long mis = (long long)(((uintptr_t)fp.base + (uintptr_t)((long long)src_slot * fp.slot_bytes)) % (uintptr_t)fp.w);
      fp.head = (int)std::min<long long>((fp.w - mis) % fp.w, fp.nbytes);
      const long long per_pass = (long long)FORK_NT * FORK_UNROLL * fp.w;
      passes = std::max(passes, (fp.nbytes - fp.head + per_pass - 1) / per_pass);
    }
    const unsigned gx = (unsigned)std::min<long long>(passes, 4096);      // (a longer plane is walked in strides of the grid)
    for (int d0 = 0; d0 < n_dst; d0 += FORK_DSTS) {
      a.n_dst = std::min(FORK_DSTS, n_dst - d0);
      for (int d = 0; d < a.n_dst; ++d) a.dst[d] = dst_slots[d0 + d];
      hipLaunchKernelGGL(td_kv_fork_kernel, dim3(gx, np), dim3(FORK_NT), 0, st, a);
      TD_CHECK_LAUNCH();
    }
  }
  return 0;
}

}  // extern "C"
