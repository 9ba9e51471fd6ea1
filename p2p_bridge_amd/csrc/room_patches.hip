// room_patches.hip -- every patch of a room in a few launches (denoise_room.py create_patches_batched; the loop it replaces,
// create_patches, issues one batch-1 FPS launch per subset and one host synchronisation per padded patch):
//   * room_fps_jobs_kernel: ragged FPS jobs, one workgroup per job. A job's cloud is points[idx_flat[off .. off + L)],
//     gathered through the radius list by the job itself (the host makes no per-job copy), sampled from a drawn start position;
//   * room_list_bounds_kernel: the bounding box of every radius list (the jitter level of the padded patches);
//   * room_assemble_kernel: xyz / idx of both kinds of patch from the picks, the duplicate draws and the jitter.
//
// The FPS is _fps_from + fps_kernel (sampling.hip) bit for bit: FPS of m samples on the list with positions 0 and `start`
// swapped, picks mapped back. The swap is virtual: LOGICAL position k' reads list position (k' == 0 ? start : k' == start ? 0 : k')
// -- an involution, so the same map turns a picked logical position into the list position that is written out. Everything
// that decides a pick is fps_kernel's: first pick logical 0, running minimum 1e38f, sqdist3, the bare v_min_f32, and the
// winner = the maximum of fps_key(best, k') (fps_key.h: the tie order of the reference's 512-thread block, over the LOGICAL
// positions). Thread t owns k' = t + 512 i: one residue class, ascending, so "first strict maximum" inside a thread agrees with
// the key order, as in fps_kernel with 512 threads.
//
// Unlike fps_kernel there are thousands of workgroups, so what a job keeps on the CU is sized for several jobs per CU: no
// coordinate cache in LDS (768 bytes of LDS per job: the waves' keys and the waves' winners' coordinates). The winner's
// coordinates ride along with its key instead: the wave's winning lane is found by ballot, its slot index is wave-uniform
// after a readlane, and the coordinates are read out of that lane's registers -- no dependent global load (list, then
// point) on the round's critical path.
//
// Tiers (points per lane of 512 threads; registers: 4 PPT for coordinates and minima + the round's temporaries). What limits the
// jobs per CU is the register file (512 VGPRs per lane and SIMD; a job is 8 waves = 2 per SIMD) or the cap of 32 waves per CU,
// never LDS. VGPRs and waves per SIMD as compiled (hipcc -Rpass-analysis=kernel-resource-usage):
//     L <=  1024   PPT  2     22 VGPRs   8 waves / SIMD   4 jobs / CU (the 32-wave cap)
//     L <=  4096   PPT  8     61 VGPRs   8 waves / SIMD   4 jobs / CU (the same cap)
//     L <=  8192   PPT 16    117 VGPRs   4 waves / SIMD   2 jobs / CU
//     L <= 16384   PPT 32    141 VGPRs   3 waves / SIMD   1 job  / CU (the 128 registers of its points alone rule out a second)
//     longer       streaming  40 VGPRs   8 waves / SIMD   2 jobs / CU of 1024 threads (the 32-wave cap); the list's points are
//                                         gathered ONCE into (x, y, z, running minimum) records in the caller's workspace and
//                                         streamed from L2 every round
// A room at the PVDL settings (patches of 4096 points) has its FPS jobs in the upper three: lists of 4096 .. 20 000 points.
// No float atomics anywhere: two runs give the same bits.
#include "common.h"
#include "fps_key.h"

#define RP_THREADS 512
#define RP_STREAM_THREADS 1024
#define RP_TIERS 5  // four register tiers + the streaming form
static const int rp_tier_cap[RP_TIERS] = {1024, 4096, 8192, 16384, 0x1FFFFFFF};  // (fps_key: k < 2^29)

// job table row: list offset into idx_flat, list length L, start position in [0, L), output row, workspace offset (floats, a
// multiple of 4; streaming: the job owns 4 L floats there)
#define RP_JOB_COLS 5

typedef float rp_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int rp_swap(int k, int start) { return k == 0 ? start : (k == start ? 0 : k); }
__device__ __forceinline__ float rp_readlane(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// PPT > 0: L <= 512 PPT, coordinates and minima in registers. PPT == 0: any L; the job first gathers its list into
// (x, y, z, running minimum) records in ws, and a round streams them from L2, four loads in flight per thread (a thread
// only ever reads the records it wrote itself).
template <int PPT>
__global__ __launch_bounds__(PPT > 0 ? RP_THREADS : RP_STREAM_THREADS) void room_fps_jobs_kernel(
    int m, int n, const float *__restrict__ points, const int *__restrict__ idx_flat, long long idx_len,
    const long long *__restrict__ table, int rows, float *__restrict__ ws, long long ws_floats, int *__restrict__ picks) {
  constexpr bool STREAM = PPT == 0;
  constexpr int THREADS = STREAM ? RP_STREAM_THREADS : RP_THREADS;
  constexpr int NP = STREAM ? 2 : PPT;  // (streaming: the register arrays are unused)
  typedef float vf __attribute__((ext_vector_type(NP)));  // (a vector, not an array: the winner's slot is a wave-uniform dynamic index)
  __shared__ u64 slots[2 * 16];                                     // per-wave maxima, double-buffered by round parity
  __shared__ __attribute__((aligned(16))) float sxyz[2][16][4];     // ... and the coordinates of those points
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long *job = table + (size_t)blockIdx.x * RP_JOB_COLS;
  const long long off = job[0], L64 = job[1], st64 = job[2], row = job[3], wso = job[4];
  // a malformed row writes nothing and reads nothing (the host wrapper checks the same on its copy of the table)
  if (off < 0 || L64 < 1 || L64 > (STREAM ? 0x1FFFFFFFLL : (long long)THREADS * PPT) || off + L64 > idx_len || st64 < 0 || st64 >= L64 ||
      row < 0 || row >= rows)
    return;
  if (STREAM && (wso < 0 || (wso & 3) != 0 || wso + 4 * L64 > ws_floats)) return;
  const int L = (int)L64, start = (int)st64;
  const int *list = idx_flat + off;
  int *out = picks + (size_t)row * m;
  rp_f32x4 *rec = STREAM ? (rp_f32x4 *)(ws + wso) : nullptr;

  // logical position k -> (x, y, z, initial running minimum); a list entry outside the room counts as "no point here"
  auto load = [&](int k) -> rp_f32x4 {
    const int ri = list[rp_swap(k, start)];
    const bool ok = (unsigned)ri < (unsigned)n;
    // 1e38: PN2/pvcnn_sampling.cpp:56 ; -1 = "no point here": v_min_f32 keeps it, and it is never selected
    return rp_f32x4{ok ? points[(size_t)ri * 3] : 0.0f, ok ? points[(size_t)ri * 3 + 1] : 0.0f, ok ? points[(size_t)ri * 3 + 2] : 0.0f,
                    ok ? 1e38f : -1.0f};
  };

  vf x, y, z, dist;
  if (!STREAM) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int k = t + i * THREADS;
      const rp_f32x4 r = k < L ? load(k) : rp_f32x4{0.0f, 0.0f, 0.0f, -1.0f};
      x[i] = r[0], y[i] = r[1], z[i] = r[2], dist[i] = r[3];
    }
  } else {
    for (int k = t; k < L; k += THREADS) rec[k] = load(k);
  }
  if (t < 32) slots[t] = 0;
  if (t == 0) out[0] = start;  // logical 0
  const rp_f32x4 first = load(0);
  float sx = first[0], sy = first[1], sz = first[2];
  __syncthreads();

  for (int j = 1; j < m; ++j) {
    // the round of fps_kernel for one point: the new running minimum (bare v_min_f32: see fps_kernel)
    auto update = [&](float px, float py, float pz, float dold) { return vmin_raw(sqdist3(px - sx, py - sy, pz - sz), dold); };
    float best = -1.0f, wx, wy, wz;
    u64 wkey;
    if (!STREAM) {
      int bi = 0;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const float d2 = update(x[i], y[i], z[i], dist[i]);
        dist[i] = d2;
        if (d2 > best) {
          best = d2;
          bi = i;
        }
      }
      const u64 key = fps_key(best, t + bi * THREADS);
      wkey = max_u64<true>(key);
      const int wl = __builtin_ctzll(__ballot(key == wkey));  // (keys are unique: the position is part of them)
      const int sbi = __builtin_amdgcn_readlane(bi, wl);      // wave-uniform: x[sbi] is a register-indexed move, not PPT selects
      wx = rp_readlane(x[sbi], wl), wy = rp_readlane(y[sbi], wl), wz = rp_readlane(z[sbi], wl);
    } else {
      float bx = 0.0f, by = 0.0f, bz = 0.0f;
      int bk = 0;
      for (int k0 = t; k0 < L; k0 += 4 * THREADS) {  // (ascending k inside the thread: its first strict maximum is the key order's)
        rp_f32x4 r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k0 + q * THREADS < L) r[q] = rec[k0 + q * THREADS];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = k0 + q * THREADS;
          if (k < L) {
            const float d2 = update(r[q][0], r[q][1], r[q][2], r[q][3]);
            if (d2 != r[q][3]) ws[wso + 4 * (long long)k + 3] = d2;
            if (d2 > best) {
              best = d2;
              bk = k;
              bx = r[q][0], by = r[q][1], bz = r[q][2];
            }
          }
        }
      }
      const u64 key = fps_key(best, bk);
      wkey = max_u64<true>(key);
      const int wl = __builtin_ctzll(__ballot(key == wkey));
      wx = rp_readlane(bx, wl), wy = rp_readlane(by, wl), wz = rp_readlane(bz, wl);
    }
    // the wave's maximum and that point's coordinates (one 16-byte store: three adjacent floats would become a ds_write_b96
    // -- tests/test_abi.py), ONE barrier, and a 16-entry row reduction that every wave repeats
    if (lane == 0) {
      slots[(j & 1) * 16 + wave] = wkey;
      *(volatile rp_f32x4 *)&sxyz[j & 1][wave][0] = rp_f32x4{wx, wy, wz, 0.0f};
    }
    __syncthreads();
    const u64 mine = slots[(j & 1) * 16 + (t & 15)];  // entries beyond the last wave stay 0 (identity)
    const u64 fin = max_u64<false>(mine);
    const int wsel = __builtin_ctzll(__ballot(lane < 16 && mine == fin));
    const rp_f32x4 sq = *(volatile rp_f32x4 *)&sxyz[j & 1][wsel][0];
    sx = sq[0], sy = sq[1], sz = sq[2];
    if (t == 0) out[j] = rp_swap(fps_key_index(fin), start);
  }
}

extern "C" int p2pb_room_fps_tier_capacity(int tier) { return tier >= 0 && tier < RP_TIERS ? rp_tier_cap[tier] : 0; }
extern "C" size_t p2pb_room_fps_jobs_ws_bytes(long long stream_points) {
  return stream_points > 0 ? (size_t)stream_points * 4 * sizeof(float) : 0;  // (x, y, z, running minimum) per point
}

extern "C" int p2pb_room_fps_jobs(int tier, int jobs, int m, int n, const float *points, const int *idx_flat, long long idx_len,
                                  const long long *table, int rows, float *ws, long long ws_floats, int *picks, void *stream) {
  if (tier < 0 || tier >= RP_TIERS || jobs <= 0 || m <= 0 || n <= 0 || idx_len <= 0 || rows <= 0 || !points || !idx_flat || !table ||
      !picks || ws_floats < 0 || (tier == RP_TIERS - 1 && (!ws || ws_floats <= 0 || ((uintptr_t)ws & 15) != 0)))
    return P2PB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
#define RP_LAUNCH(PPT)                                                                                                     \
  hipLaunchKernelGGL(room_fps_jobs_kernel<PPT>, dim3(jobs), dim3(PPT > 0 ? RP_THREADS : RP_STREAM_THREADS), 0, s, m, n, points, \
                     idx_flat, idx_len, table, rows, ws, ws_floats, picks)
  switch (tier) {
    case 0: RP_LAUNCH(2); break;
    case 1: RP_LAUNCH(8); break;
    case 2: RP_LAUNCH(16); break;
    case 3: RP_LAUNCH(32); break;
    default: RP_LAUNCH(0); break;
  }
#undef RP_LAUNCH
  return p2pb_launch_status();
}

// bounds[c] = (min x, y, z, max x, y, z) over points[idx_flat[offsets[c] .. offsets[c + 1])], exact fp32; one wave per list
// (an empty list: +inf / -inf). Entries outside the room are passed over.
__global__ __launch_bounds__(256) void room_list_bounds_kernel(int s, int n, const float *__restrict__ points,
                                                               const int *__restrict__ idx_flat,
                                                               const long long *__restrict__ offsets, long long idx_len,
                                                               float *__restrict__ bounds) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= s) return;
  const int lane = lane_id();
  long long a = offsets[c], b = offsets[c + 1];
  if (a < 0) a = 0;
  if (b > idx_len) b = idx_len;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long i = a + lane; i < b; i += 64) {
    const int ri = idx_flat[i];
    if ((unsigned)ri >= (unsigned)n) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = points[(size_t)ri * 3 + d];
      lo[d] = fminf(lo[d], v);
      hi[d] = fmaxf(hi[d], v);
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[d] = fminf(lo[d], __shfl_xor(lo[d], o));
      hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o));
    }
  }
  if (lane < 6) bounds[(size_t)c * 6 + lane] = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lane == 2 ? lo[2] : lane == 3 ? hi[0] : lane == 4 ? hi[1] : hi[2];
}

extern "C" int p2pb_room_list_bounds(int s, int n, const float *points, const int *idx_flat, long long idx_len,
                                     const long long *offsets, float *bounds, void *stream) {
  if (s <= 0 || n <= 0 || idx_len < 0 || !points || !idx_flat || !offsets || !bounds) return P2PB_EINVAL;
  hipLaunchKernelGGL(room_list_bounds_kernel, dim3(cdiv(s, 4)), dim3(256), 0, (hipStream_t)stream, s, n, points, idx_flat, offsets,
                     idx_len, bounds);
  return p2pb_launch_status();
}

// patch table row: list offset, list length L, source, kind. kind 1 (FPS patch): source = its row of picks, entry j is list
// position picks[source][j]. kind 0 (padded patch, L < k): entries j < L are the list in order, entry L + q is the duplicate
// list position pad_r[source + q] moved by jitter[source + q] (one fp32 add per coordinate).
#define RP_PATCH_COLS 4
__global__ __launch_bounds__(256) void room_assemble_kernel(int npatch, int k, int n, const float *__restrict__ points,
                                                            const int *__restrict__ idx_flat, long long idx_len,
                                                            const long long *__restrict__ table, const int *__restrict__ picks,
                                                            int rows, const long long *__restrict__ pad_r,
                                                            const float *__restrict__ jitter, long long pad_total,
                                                            float *__restrict__ xyz, long long *__restrict__ idx) {
  const int p = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
  if (p >= npatch || j >= k) return;
  const long long *row = table + (size_t)p * RP_PATCH_COLS;
  const long long off = row[0], L = row[1], src = row[2], kind = row[3];
  long long pos = -1, q = -1;
  if (kind == 1) {
    if (src >= 0 && src < rows) pos = picks[(size_t)src * k + j];
  } else if (j < L) {
    pos = j;
  } else {
    q = src + (j - L);
    if (src >= 0 && q < pad_total) pos = pad_r[q];
    else q = -1;
  }
  long long ri = -1;
  if (pos >= 0 && pos < L && off >= 0 && off + pos < idx_len) ri = idx_flat[off + pos];
  const bool ok = ri >= 0 && ri < n;  // (a malformed row or entry: index -1 and NaN coordinates, never a stray read)
  const size_t o = (size_t)p * k + j;
  idx[o] = ok ? ri : -1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    float v = ok ? points[(size_t)ri * 3 + d] : NAN;
    if (ok && q >= 0) v = v + jitter[(size_t)q * 3 + d];
    xyz[o * 3 + d] = v;
  }
}

extern "C" int p2pb_room_assemble_patches(int npatch, int k, int n, const float *points, const int *idx_flat, long long idx_len,
                                          const long long *table, const int *picks, int rows, const long long *pad_r,
                                          const float *jitter, long long pad_total, float *xyz, long long *idx, void *stream) {
  if (npatch <= 0 || k <= 0 || k > 65535 * 256 || n <= 0 || idx_len <= 0 || rows < 0 || pad_total < 0 || !points || !idx_flat || !table ||
      !xyz || !idx || (rows > 0 && !picks) || (pad_total > 0 && (!pad_r || !jitter)))
    return P2PB_EINVAL;
  hipLaunchKernelGGL(room_assemble_kernel, dim3(npatch, cdiv(k, 256)), dim3(256), 0, (hipStream_t)stream, npatch, k, n, points,
                     idx_flat, idx_len, table, picks, rows, pad_r, jitter, pad_total, xyz, idx);
  return p2pb_launch_status();
}
