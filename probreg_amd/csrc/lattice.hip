// GPU permutohedral lattice on MI355X (gfx950): parallel hash build, atomic / ordered splat, blur, slice - the stand-alone
// filter (prg_ph_*: gaussian_filtering.Permutohedral, the FPFH feature path) and the E-step of the FilterReg plan (filterreg.hip).
//
// Reference behaviour (neka-nat/probreg v0.3.7):
//   lattice   third_party/permutohedral/permutohedral.cpp:140-325 (init, SSE build) and :482-616 (compute)
//             behind probreg/gaussian_filtering.py:8-17 / probreg/cc/permutohedral_lattice_py.cc:13-21
//
// The embedding arithmetic (elevate, round-half-even, rank, barycentric) is evaluated in float32 with
// explicitly un-fused operations so that every point lands in the same simplex with the same weights as
// in the reference's SSE build; vertex ids are arbitrary labels (hash order), which no output depends on.
// The splat is a float atomic add, i.e. the summation ORDER differs from the reference's sequential loop
// (float32 round-off only).  Everything here is HBM-latency / atomic bound integer and scatter work.
#include <math.h>

#include <algorithm>
#include <new>
#include <type_traits>

#include <stdio.h>
#include <stdlib.h>

#include "prg_device.h"
#include "prg_common.h"
#include "lattice.h"
#include "lattice_sort.h"

using prg::FrFeat;
using prg::LatticeMail;

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kEmpty = 0xFFFFFFFFFFFFFFFFull;
constexpr int kMaxD = 3;

__device__ __forceinline__ unsigned long long pack_key(const short* k, int d) {
    unsigned long long r = 0;
    for (int i = 0; i < d; ++i) r |= (unsigned long long)(unsigned short)k[i] << (16 * i);
    return r;
}
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// ---- embedding (permutohedral.cpp:186-276, SSE build) -------------------------------------------------
// One hash table of a lattice build: entries are (generation << 48) | packed key (see Lattice::gen).
struct EmbedTable {
    unsigned long long* tkeys;
    unsigned long long mask;
    unsigned gen;
    int* count;               // [0] vertices created so far, [1] overflow flag
    int* slot_id;             // may be null (count only)
    unsigned long long* dkeys;
};

// Embed one point (features f, scale factors s) and insert its D + 1 vertices into table T.  pslot_i / bary_i: where the
// point's slots and barycentric weights go, or null (the side table of the speculative with_blur decision only counts).
template <int D>
__device__ __forceinline__ void embed_insert(const float (&f)[D], float s0, float s1, float s2, const EmbedTable& T,
                                             int lane, int* __restrict__ pslot_i, float* __restrict__ bary_i) {
    constexpr int D1 = D + 1;
    unsigned long long* __restrict__ tkeys = T.tkeys;
    const unsigned long long mask = T.mask;
    const unsigned gen = T.gen;
    int* __restrict__ count = T.count;
    int* __restrict__ slot_id = T.slot_id;
    unsigned long long* __restrict__ dkeys = T.dkeys;
    const unsigned long long gbits = (unsigned long long)gen << 48;
    const float scale[3] = {s0, s1, s2};
    float elevated[D1], rem0[D1], rank[D1], bar[D1 + 1];
    float sm = 0.f;
#pragma unroll
    for (int j = D; j > 0; --j) {
        const float cf = __fmul_rn(f[j - 1], scale[j - 1]);
        elevated[j] = __fsub_rn(sm, __fmul_rn((float)j, cf));
        sm = __fadd_rn(sm, cf);
    }
    elevated[0] = sm;
    const float invd1 = 1.0f / (float)D1, fd1 = (float)D1;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < D1; ++k) {
        float v = __fmul_rn(invd1, elevated[k]);
        v = rintf(v);  // round half to even (_mm_cvtps_epi32 under the default MXCSR, :214-218)
        rem0[k] = __fmul_rn(v, fd1);
        sum = __fadd_rn(sum, v);
    }
#pragma unroll
    for (int k = 0; k < D1; ++k) rank[k] = 0.f;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const float da = __fsub_rn(elevated[a], rem0[a]);
#pragma unroll
        for (int b = a + 1; b < D1; ++b) {
            const float db = __fsub_rn(elevated[b], rem0[b]);
            if (da < db) rank[a] += 1.f; else rank[b] += 1.f;
        }
    }
#pragma unroll
    for (int k = 0; k < D1; ++k) {
        rank[k] += sum;
        if (rank[k] < 0.f) { rank[k] += fd1; rem0[k] += fd1; }
        else if (rank[k] >= fd1) { rank[k] -= fd1; rem0[k] -= fd1; }
    }
#pragma unroll
    for (int k = 0; k <= D1; ++k) bar[k] = 0.f;
#pragma unroll
    for (int k = 0; k < D1; ++k) {
        const float v = __fmul_rn(__fsub_rn(elevated[k], rem0[k]), invd1);
        const int p = D - (int)rank[k];
#pragma unroll
        for (int q = 0; q <= D1; ++q) {  // static indexing keeps bar[] in registers
            if (q == p) bar[q] = __fadd_rn(bar[q], v);
            if (q == p + 1) bar[q] = __fsub_rn(bar[q], v);
        }
    }
    bar[0] = __fadd_rn(bar[0], __fadd_rn(1.0f, bar[D1]));
    unsigned nclaim_mask = 0;  // rounds in which this lane created a vertex, with the slot and key of each
    int fslot[D1];             // the slot every round ended on
    int cslot[D1];
    unsigned long long ckey[D1];
#pragma unroll
    for (int r = 0; r < D1; ++r) {
        cslot[r] = 0;
        ckey[r] = 0;
    }
#pragma unroll
    for (int r = 0; r < D1; ++r) {
        short key[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            // canonical[r][rank] = r if rank <= D - r else r - (D+1)   (:166-171)
            const int rk = (int)rank[k];
            const int can = (rk <= D - r) ? r : r - D1;
            key[k] = (short)(rem0[k] + (float)can);
        }
        const unsigned long long pk = pack_key(key, D), mine = pk | gbits;
        unsigned long long slot = mix64(pk) & mask;
        bool claimed = false;
        for (int probes = 0;; ++probes) {
            if (probes > 4096) {  // table (sized from the previous lattice) is too small: the host rebuilds
                count[1] = 1;
                slot = 0;
                break;
            }
            // An ordinary (cacheable) read first: it may be stale - each XCD has its own L2, coherent with the others only
            // at kernel boundaries - but an entry of THIS generation never changes once written, so a hit or a slot taken
            // by another key of this build is final, and only a slot that LOOKS free is asked again at device scope
            // (that read goes past the L2s to the memory side and costs several times as much).  Once a vertex exists,
            // the ~N/L points sharing it never issue an atomic - a CAS storm on a few hundred hot keys costs milliseconds
            // when sigma is large.
            unsigned long long cur = tkeys[slot];
            if (cur == mine) break;
            if ((unsigned)(cur >> 48) != gen)
                cur = __hip_atomic_load(&tkeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)(cur >> 48) != gen) {  // empty, or left over from an earlier build
                const unsigned long long old = atomicCAS(&tkeys[slot], cur, mine);
                if (old == cur) {
                    claimed = true;
                    break;
                }
                cur = old;  // somebody of this build got there first
            }
            if (cur == mine) break;
            slot = (slot + 1) & mask;
        }
        if (claimed) {
            nclaim_mask |= 1u << r;
            cslot[r] = (int)slot;
            ckey[r] = pk;
        }
        fslot[r] = (int)slot;
    }
    if (pslot_i) {
        // [r5] D = 3: one 16-byte store per point and array (a wave writes 1 KB contiguous) instead of four 4-byte stores at a
        // stride of 16 bytes each
        if constexpr (D1 == 4) {
            *reinterpret_cast<int4*>(pslot_i) = make_int4(fslot[0], fslot[1], fslot[2], fslot[3]);
            *reinterpret_cast<float4*>(bary_i) = make_float4(bar[0], bar[1], bar[2], bar[3]);
        } else {
#pragma unroll
            for (int r = 0; r < D1; ++r) {
                pslot_i[r] = fslot[r];
                bary_i[r] = bar[r];
            }
        }
    }
    // whoever created a vertex numbers it (no scan of the table afterwards): ONE counter update per wave - the lanes'
    // claims of all D + 1 rounds are ranked with ballots, the first claiming lane fetches the base
    unsigned long long bal[D1];
    int total = 0;
#pragma unroll
    for (int r = 0; r < D1; ++r) {
        bal[r] = __ballot((nclaim_mask >> r) & 1u);
        total += __popcll(bal[r]);
    }
    if (total) {
        unsigned long long any = 0;
#pragma unroll
        for (int r = 0; r < D1; ++r) any |= bal[r];
        const int leader = __ffsll((long long)any) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(count, total);
        base = __shfl(base, leader, 64);
        if (slot_id) {
            int before = 0;
#pragma unroll
            for (int r = 0; r < D1; ++r) {
                if ((nclaim_mask >> r) & 1u) {
                    const int id = base + before + __popcll(bal[r] & ((1ull << lane) - 1ull));
                    slot_id[cslot[r]] = id;
                    dkeys[id] = ckey[r];
                }
                before += __popcll(bal[r]);
            }
        }
    }
}

// side.tkeys != null: the same points are ALSO embedded with the scale factors (t0, t1, t2) into the side table (count
// only) - the speculative with_blur decision of prg_fr_estep rides in the first launch of the build instead of its own.
template <int D, bool FR>
__global__ __launch_bounds__(kBlock) void k_embed(const float* __restrict__ feat, const FrFeat fr, int64_t first,
                                                  int64_t n, float s0, float s1, float s2, const EmbedTable table,
                                                  int* __restrict__ pslot, float* __restrict__ bary,
                                                  const EmbedTable side, float t0, float t1, float t2, int sample) {
    // sample 0: points [first, n); 1: every 16th point of [0, n) (a sample spread over the whole cloud: it creates most
    // vertices with few lanes of a wave after the same one); 2: all the others
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int period = sample >> 2;  // stage 1 takes every period-th point (sample & 3 == 1), stage 2 the others (== 2)
    sample &= 3;
    const int64_t i = sample == 0 ? first + t : (sample == 1 ? (int64_t)period * t : t + t / (period - 1) + 1);
    if (i >= n) return;
    constexpr int D1 = D + 1;
    const int lane = threadIdx.x & 63;
    float f[D];
    if (FR) {
        const double sigma = sqrt(fr.state[12]);
        if (i < fr.m) {
            // [r5] source / target / transformed source are stored 4 doubles per point (x, y, z, 0): two 16-byte accesses per
            // point that a wave issues over contiguous memory, instead of three 8-byte ones at a stride of 24 bytes
            const double2 ya = reinterpret_cast<const double2*>(fr.src)[2 * i], yb = reinterpret_cast<const double2*>(fr.src)[2 * i + 1];
            const double y[3] = {ya.x, ya.y, yb.x};
            double zt[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) acc += y[k] * fr.state[3 * r + k];  // dot(points, rot.T), transformation.py:49-50
                const double z = r < D ? acc + fr.state[9 + r] : 0.0;
                zt[r] = z;
                if (r < D) f[r < D ? r : 0] = (float)(z / sigma);
            }
            reinterpret_cast<double2*>(fr.ts)[2 * i] = make_double2(zt[0], zt[1]);
            reinterpret_cast<double2*>(fr.ts)[2 * i + 1] = make_double2(zt[2], 0.0);
        } else {
            const double2 xa = reinterpret_cast<const double2*>(fr.tgt)[2 * (i - fr.m)], xb = reinterpret_cast<const double2*>(fr.tgt)[2 * (i - fr.m) + 1];
            const double xt[3] = {xa.x, xa.y, xb.x};
#pragma unroll
            for (int k = 0; k < D; ++k) f[k] = (float)(xt[k] / sigma);
        }
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) f[k] = feat[i * D + k];
    }
    embed_insert<D>(f, s0, s1, s2, table, lane, pslot + i * D1, bary + i * D1);
    if (side.tkeys) embed_insert<D>(f, t0, t1, t2, side, lane, nullptr, nullptr);
}

// ---- feature-space lattices, d > 3 (filterreg.py:121, 125-133 with feature_fn = FPFH: d = 33) ---------------------
// The same embedding with run-time d (arrays of d + 1 floats per thread, in scratch).  A key is d shorts and does not fit
// a machine word, so the table stores a 64-bit hash of it; a SECOND, independent 64-bit hash is recorded per vertex and
// checked by every point that lands on the vertex and by every neighbour look-up: two different keys that share a table
// hash are detected (the host then rebuilds with other seeds) instead of silently merged.
constexpr int kMaxDG = 64;
__device__ __forceinline__ unsigned long long hash_shorts(const short* key, int d, unsigned long long seed) {
    unsigned long long h = seed;
    for (int i = 0; i < d; ++i) {
        h ^= (unsigned long long)(unsigned short)key[i];
        h *= 0x100000001b3ull;
        h ^= h >> 29;
    }
    h = mix64(h);
    return h == kEmpty ? h - 1 : h;
}
__device__ __forceinline__ short canonical_key(float rem0, int rk, int r, int d) {
    // canonical[r][rank] = r if rank <= d - r else r - (d + 1)   (permutohedral.cpp:166-171)
    return (short)(rem0 + (float)(rk <= d - r ? r : r - (d + 1)));
}

__global__ __launch_bounds__(kBlock) void k_embed_g(const float* __restrict__ feat, int64_t n, int d,
                                                    const float* __restrict__ scale,
                                                    unsigned long long* __restrict__ tkeys, unsigned long long mask,
                                                    unsigned long long seed, int* __restrict__ pslot,
                                                    float* __restrict__ bary, short* __restrict__ rem0s,
                                                    unsigned char* __restrict__ rank8, int* __restrict__ overflow) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int d1 = d + 1;
    float elevated[kMaxDG + 1], rem0[kMaxDG + 1], rank[kMaxDG + 1], bar[kMaxDG + 2];
    float sm = 0.f;
    for (int j = d; j > 0; --j) {
        const float cf = __fmul_rn(feat[i * d + j - 1], scale[j - 1]);
        elevated[j] = __fsub_rn(sm, __fmul_rn((float)j, cf));
        sm = __fadd_rn(sm, cf);
    }
    elevated[0] = sm;
    const float invd1 = 1.0f / (float)d1, fd1 = (float)d1;
    float sum = 0.f;
    for (int k = 0; k < d1; ++k) {
        float v = rintf(__fmul_rn(invd1, elevated[k]));  // round half to even, as in k_embed
        rem0[k] = __fmul_rn(v, fd1);
        sum = __fadd_rn(sum, v);
        rank[k] = 0.f;
    }
    for (int a = 0; a < d; ++a) {
        const float da = __fsub_rn(elevated[a], rem0[a]);
        for (int b = a + 1; b < d1; ++b) {
            const float db = __fsub_rn(elevated[b], rem0[b]);
            if (da < db) rank[a] += 1.f; else rank[b] += 1.f;
        }
    }
    for (int k = 0; k < d1; ++k) {
        rank[k] += sum;
        if (rank[k] < 0.f) { rank[k] += fd1; rem0[k] += fd1; }
        else if (rank[k] >= fd1) { rank[k] -= fd1; rem0[k] -= fd1; }
    }
    for (int k = 0; k <= d1; ++k) bar[k] = 0.f;
    for (int k = 0; k < d1; ++k) {
        const float v = __fmul_rn(__fsub_rn(elevated[k], rem0[k]), invd1);
        const int p = d - (int)rank[k];
        bar[p] = __fadd_rn(bar[p], v);
        bar[p + 1] = __fsub_rn(bar[p + 1], v);
    }
    bar[0] = __fadd_rn(bar[0], __fadd_rn(1.0f, bar[d1]));
    for (int k = 0; k < d1; ++k) {
        rem0s[i * d1 + k] = (short)rem0[k];
        rank8[i * d1 + k] = (unsigned char)(int)rank[k];
    }
    for (int r = 0; r < d1; ++r) {
        short key[kMaxDG];
        for (int k = 0; k < d; ++k) key[k] = canonical_key(rem0[k], (int)rank[k], r, d);
        const unsigned long long pk = hash_shorts(key, d, seed);
        unsigned long long slot = mix64(pk) & mask;
        for (int probes = 0;; ++probes) {
            if (probes > 4096) {
                *overflow = 1;
                slot = 0;
                break;
            }
            unsigned long long cur = __hip_atomic_load(&tkeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kEmpty) cur = atomicCAS(&tkeys[slot], kEmpty, pk);
            if (cur == kEmpty || cur == pk) break;
            slot = (slot + 1) & mask;
        }
        pslot[i * d1 + r] = (int)slot;
        bary[i * d1 + r] = bar[r];
    }
}

// After compaction / resolve: every (point, remainder) writes its key into its vertex' row of kfull (all writers of a
// vertex write the same d shorts) and checks the vertex' second hash.  flag[0] = 1 on a table-hash collision.
__global__ __launch_bounds__(kBlock) void k_store_keys_g(const int* __restrict__ offset, int64_t n, int d,
                                                         const short* __restrict__ rem0s,
                                                         const unsigned char* __restrict__ rank8,
                                                         unsigned long long seed2, short* __restrict__ kfull,
                                                         unsigned long long* __restrict__ gcheck, int* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int d1 = d + 1;
    if (t >= n * d1) return;
    const int64_t i = t / d1;
    const int r = (int)(t % d1);
    const int id = offset[t];
    short key[kMaxDG];
    for (int k = 0; k < d; ++k) key[k] = canonical_key((float)rem0s[i * d1 + k], (int)rank8[i * d1 + k], r, d);
    const unsigned long long g = hash_shorts(key, d, seed2) | 1ull;
    const unsigned long long old = atomicCAS(&gcheck[id], 0ull, g);
    if (old == 0ull) {
        for (int k = 0; k < d; ++k) kfull[(int64_t)id * d + k] = key[k];
    } else if (old != g) {
        *flag = 1;
    }
}

__device__ __forceinline__ int lookup_g(const unsigned long long* __restrict__ tkeys, unsigned long long mask,
                                        const int* __restrict__ slot_id, const unsigned long long* __restrict__ gcheck,
                                        const short* key, int d, unsigned long long seed, unsigned long long seed2,
                                        int* __restrict__ flag) {
    const unsigned long long pk = hash_shorts(key, d, seed);
    unsigned long long slot = mix64(pk) & mask;
    for (;;) {
        const unsigned long long k = tkeys[slot];
        if (k == pk) {
            const int id = slot_id[slot];
            if (gcheck[id] != (hash_shorts(key, d, seed2) | 1ull)) *flag = 1;  // same table hash, different key
            return id;
        }
        if (k == kEmpty) return -1;
        slot = (slot + 1) & mask;
    }
}

// blur neighbours (permutohedral.cpp:300-324) from the full keys
__global__ __launch_bounds__(kBlock) void k_neighbours_g(const short* __restrict__ kfull, int size, int d,
                                                         const unsigned long long* __restrict__ tkeys,
                                                         unsigned long long mask, const int* __restrict__ slot_id,
                                                         const unsigned long long* __restrict__ gcheck,
                                                         unsigned long long seed, unsigned long long seed2,
                                                         int* __restrict__ nb1, int* __restrict__ nb2,
                                                         int* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)size * (d + 1)) return;
    const int j = (int)(t / size), v = (int)(t % size);
    short n1[kMaxDG], n2[kMaxDG];
    for (int k = 0; k < d; ++k) {
        const short key = kfull[(int64_t)v * d + k];
        n1[k] = (short)(k == j ? key + d : key - 1);
        n2[k] = (short)(k == j ? key - d : key + 1);
    }
    nb1[(int64_t)j * size + v] = lookup_g(tkeys, mask, slot_id, gcheck, n1, d, seed, seed2, flag);
    nb2[(int64_t)j * size + v] = lookup_g(tkeys, mask, slot_id, gcheck, n2, d, seed, seed2, flag);
}

// Dense vertex ids for the occupied slots.  One atomic per workgroup (wave ballot + LDS prefix): a lattice of a few
// hundred thousand vertices otherwise serialises that many same-address atomics (~5 ns each).
__global__ __launch_bounds__(kBlock) void k_compact(const unsigned long long* __restrict__ tkeys, int64_t cap,
                                                    int* __restrict__ slot_id, unsigned long long* __restrict__ dkeys,
                                                    int* __restrict__ count) {
    __shared__ int wave_cnt[kBlock / 64];
    __shared__ int block_base;
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long k = s < cap ? tkeys[s] : kEmpty;
    const bool occ = k != kEmpty;
    const unsigned long long bal = __ballot(occ);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            const int c = wave_cnt[w];
            wave_cnt[w] = tot;
            tot += c;
        }
        block_base = tot ? atomicAdd(count, tot) : 0;
    }
    __syncthreads();
    if (occ) {
        const int id = block_base + wave_cnt[wv] + before;
        slot_id[s] = id;
        dkeys[id] = k;
    }
}

// Every (point, remainder) slot index -> the dense vertex id of the slot.  The launch needs nothing the host does not know
// before the embedding has run, so it is issued right behind it; its first thread PUBLISHES the embedding's counters (vertex
// count, overflow flag, and the side table's pair) in the host's mapped mailbox - the host learns the lattice size while this
// kernel runs and enqueues the size-dependent launches behind it, without draining the queue - and clears them for the next
// build (`mail` null: plain resolve).
__global__ __launch_bounds__(kBlock) void k_resolve(int* __restrict__ pslot, int64_t total,
                                                    const int* __restrict__ slot_id, int* __restrict__ count,
                                                    int* __restrict__ count2, LatticeMail* __restrict__ mail,
                                                    unsigned seq) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // (one int4 = four entries per thread)
    if (i == 0 && mail) {
        mail->size = count[0];
        mail->overflow = count[1];
        mail->side_size = count2 ? count2[0] : 0;
        mail->side_overflow = count2 ? count2[1] : 0;
        __threadfence_system();
        __hip_atomic_store(&mail->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        count[0] = count[1] = 0;
        if (count2) count2[0] = count2[1] = 0;
    }
    if (4 * i + 3 < total) {
        int4 v = reinterpret_cast<int4*>(pslot)[i];
        v.x = slot_id[v.x];
        v.y = slot_id[v.y];
        v.z = slot_id[v.z];
        v.w = slot_id[v.w];
        reinterpret_cast<int4*>(pslot)[i] = v;
    } else {
        for (int64_t t = 4 * i; t < total; ++t) pslot[t] = slot_id[pslot[t]];
    }
}

__device__ __forceinline__ int lookup(const unsigned long long* __restrict__ tkeys, unsigned long long mask,
                                      const int* __restrict__ slot_id, unsigned long long pk, unsigned gen) {
    unsigned long long slot = mix64(pk) & mask;
    const unsigned long long want = pk | ((unsigned long long)gen << 48);
    for (;;) {
        const unsigned long long k = tkeys[slot];
        if (k == want) return slot_id[slot];
        if ((unsigned)(k >> 48) != gen) return -1;
        slot = (slot + 1) & mask;
    }
}

// blur neighbours (permutohedral.cpp:300-324): along axis j, n1 = key - 1 (all coords) with n1[j] = key[j] + d,
// n2 = key + 1 with n2[j] = key[j] - d; axis j == d only touches the implicit last coordinate.
template <int D>
__global__ __launch_bounds__(kBlock) void k_neighbours(const unsigned long long* __restrict__ dkeys, int size,
                                                       const unsigned long long* __restrict__ tkeys,
                                                       unsigned long long mask, const int* __restrict__ slot_id,
                                                       int* __restrict__ nb1, int* __restrict__ nb2, unsigned gen) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)size * (D + 1)) return;
    const int j = (int)(t / size), v = (int)(t % size);
    const unsigned long long pk = dkeys[v];
    short key[D], n1[D], n2[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        key[k] = (short)(unsigned short)(pk >> (16 * k));
        n1[k] = (short)(key[k] - 1);
        n2[k] = (short)(key[k] + 1);
    }
#pragma unroll
    for (int k = 0; k < D; ++k)
        if (k == j) { n1[k] = (short)(key[k] + D); n2[k] = (short)(key[k] - D); }
    nb1[(int64_t)j * size + v] = lookup(tkeys, mask, slot_id, pack_key(n1, D), gen);
    nb2[(int64_t)j * size + v] = lookup(tkeys, mask, slot_id, pack_key(n2, D), gen);
}

// ---- filtering (permutohedral.cpp:482-616) --------------------------------------------------------------
// vals layout: [(size + 1)][C], row 0 is the all-zero row that the missing-neighbour id -1 maps to.
// FX: the terms are accumulated as 64-bit fixed-point integers (term * 2^S_k, S_k per channel from the largest |value| of the
// channel: k_chan_scale) - integer addition is associative, so the atomics' arrival order no longer matters: the same bits
// in every run, and each vertex' value is the correctly rounded EXACT sum of its terms.  !FX: float atomics (arrival order).
template <bool FX>
__device__ __forceinline__ void splat_add_global(float* __restrict__ vals, long long* __restrict__ fx, int64_t idx, float term,
                                                 double mul) {
    if (FX)
        atomicAdd(reinterpret_cast<unsigned long long*>(fx + idx), (unsigned long long)__double2ll_rn((double)term * mul));
    else
        unsafeAtomicAdd(&vals[idx], term);
}

template <bool FX>
__global__ __launch_bounds__(kBlock) void k_splat(const int* __restrict__ offset, const float* __restrict__ bary,
                                                  const float* __restrict__ in, int64_t first, int64_t n, int d1,
                                                  int ch, float* __restrict__ vals, long long* __restrict__ fx,
                                                  const double* __restrict__ scale) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (n - first) * d1) return;
    const int64_t i = first + t / d1;
    const int r = (int)(t % d1);
    const int o = offset[i * d1 + r] + 1;
    const float w = bary[i * d1 + r];
    for (int k = 0; k < ch; ++k) {
        const float p = __fmul_rn(w, in[i * ch + k]);
        if (p != 0.f) splat_add_global<FX>(vals, fx, (int64_t)o * ch + k, p, FX ? scale[k] : 0.0);
    }
}

// Block-private splat: every workgroup accumulates its chunk of points into an LDS hash table keyed by the
// vertex id (ds atomics), then flushes each occupied entry with ONE global atomic per channel.  While the
// lattice is small (sigma large: a few hundred vertices shared by 2M point-vertex incidences) this removes
// the same-address global atomic storm; when a chunk touches more distinct vertices than the table holds,
// the overflow goes straight to global memory, where contention is low by then.
// (256 points / 256 slots per workgroup: 9 KB of LDS (17 KB in fixed point), 8 workgroups per CU.  The first version used 2048 / 2048 = 72 KB:
// 245 workgroups of one wave per SIMD each, every lane walking 32 incidences through dependent loads and returning LDS
// atomics with nobody to hide the latency - 52 % of the wave cycles were waits, profiles/r2_filterreg_500k_pmc.txt)
// [r5] The table's value rows are as wide as the filter has channels (STRIDE 5 for FilterReg's point-to-point pass, 8 otherwise), and
// the five-channel table has 512 slots in the LDS the 256 x 8 one takes (22 KB in fixed point): late EM iterations, where the 1024
// incidences of a workgroup's 256 points spread over more distinct vertices than 192 slots hold, overflow to global atomics less.
constexpr int kSplatMaxCh = 8;
constexpr int kSplatPts = 256;                // points per workgroup
template <bool FX, int kSplatBits, int STRIDE>
__global__ __launch_bounds__(kBlock) void k_splat_lds(const int* __restrict__ offset, const float* __restrict__ bary,
                                                      const float* __restrict__ in, int64_t first, int64_t n, int d1,
                                                      int ch, float* __restrict__ vals, long long* __restrict__ fx,
                                                      const double* __restrict__ scale) {
    typedef typename std::conditional<FX, unsigned long long, float>::type acc_t;
    constexpr int kSplatSlots = 1 << kSplatBits;  // LDS table entries (key + STRIDE channels)
    __shared__ int skey[kSplatSlots];
    __shared__ acc_t sval[kSplatSlots * STRIDE];
    __shared__ int sfill;
    for (int t = threadIdx.x; t < kSplatSlots; t += kBlock) skey[t] = -1;
    for (int t = threadIdx.x; t < kSplatSlots * STRIDE; t += kBlock) sval[t] = (acc_t)0;
    if (threadIdx.x == 0) sfill = 0;
    __syncthreads();
    double mul[kSplatMaxCh];
#pragma unroll
    for (int k = 0; k < kSplatMaxCh; ++k) mul[k] = (FX && k < ch) ? scale[k] : 0.0;
    const int64_t p0 = first + (int64_t)blockIdx.x * kSplatPts;
    const int64_t p1 = (p0 + kSplatPts < n) ? p0 + kSplatPts : n;
    for (int64_t t = (p0 - first) * d1 + threadIdx.x; t < (p1 - first) * d1; t += kBlock) {
        const int64_t i = first + t / d1;
        const int r = (int)(t % d1);
        const float w = bary[i * d1 + r];
        const int o = offset[i * d1 + r] + 1;
        bool any = false;
        float p[kSplatMaxCh];
#pragma unroll
        for (int k = 0; k < kSplatMaxCh; ++k) {
            p[k] = k < ch ? __fmul_rn(w, in[i * ch + k]) : 0.f;
            any |= p[k] != 0.f;
        }
        if (!any) continue;
        unsigned h = ((unsigned)o * 2654435761u) >> (32 - kSplatBits);
        int slot = -1;
        for (int probe = 0; probe < 16; ++probe) {
            int cur = skey[h];
            if (cur == -1 && sfill < kSplatSlots * 3 / 4) {
                cur = atomicCAS(&skey[h], -1, o);
                if (cur == -1) { atomicAdd(&sfill, 1); cur = o; }
            }
            if (cur == o) { slot = (int)h; break; }
            h = (h + 1) & (kSplatSlots - 1);
        }
#pragma unroll
        for (int k = 0; k < kSplatMaxCh; ++k) {
            if (k >= ch || p[k] == 0.f) continue;
            if (slot >= 0) {
                if (FX)
                    atomicAdd(reinterpret_cast<unsigned long long*>(&sval[slot * STRIDE + k]),
                              (unsigned long long)__double2ll_rn((double)p[k] * mul[k]));
                else
                    atomicAdd(reinterpret_cast<float*>(&sval[slot * STRIDE + k]), p[k]);
            } else {
                splat_add_global<FX>(vals, fx, (int64_t)o * ch + k, p[k], mul[k]);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kSplatSlots; t += kBlock) {
        const int o = skey[t];
        if (o < 0) continue;
        for (int k = 0; k < ch; ++k) {
            const acc_t v = sval[t * STRIDE + k];
            if (v == (acc_t)0) continue;
            if (FX)
                atomicAdd(reinterpret_cast<unsigned long long*>(fx + (int64_t)o * ch + k), (unsigned long long)v);
            else
                unsafeAtomicAdd(&vals[(int64_t)o * ch + k], (float)v);
        }
    }
}

// largest |in[i][k]| over the splatted rows, per channel -> maxabs[k] as float bits (non-negative floats order like their
// bits); one atomic per workgroup and channel
__global__ __launch_bounds__(kBlock) void k_chan_maxabs(const float* __restrict__ in, int64_t first, int64_t n, int ch,
                                                        unsigned* __restrict__ maxabs) {
    __shared__ unsigned smax[32];
    if (threadIdx.x < 32) smax[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t total = (n - first) * ch;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t step = stride - stride % ch;  // a thread stays on one channel
    float v = 0.f;
    for (int64_t z = t; z < total; z += step) v = fmaxf(v, fabsf(in[first * ch + z]));
    if (t < total && v > 0.f && isfinite(v)) atomicMax(&smax[t % ch], __float_as_uint(v));
    __syncthreads();
    if (threadIdx.x < ch && smax[threadIdx.x]) atomicMax(maxabs + threadIdx.x, smax[threadIdx.x]);
}

// scale[k] = 2^S_k with n * maxabs_k * 2^S_k < 2^61 (no overflow whatever the vertex), scale[ch + k] = 2^-S_k
__global__ void k_chan_scale(const unsigned* __restrict__ maxabs, int ch, double n_points, double* __restrict__ scale) {
    const int k = threadIdx.x;
    if (k >= ch) return;
    const double m = (double)__uint_as_float(maxabs[k]);
    int e = 0;
    if (m > 0.0) {
        (void)frexp(m * n_points, &e);  // m n < 2^e
        e = 61 - e;
        e = e > 120 ? 120 : (e < -120 ? -120 : e);
    }
    scale[k] = ldexp(1.0, e);
    scale[ch + k] = ldexp(1.0, -e);
}

// fixed-point sums -> the float value plane a (row 0 of both planes: the all-zero row)
__global__ __launch_bounds__(kBlock) void k_fix_to_float(long long* __restrict__ fx, int64_t elems, int ch,
                                                         const double* __restrict__ scale, float* __restrict__ vals_a,
                                                         float* __restrict__ vals_b) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= elems) return;
    const int k = (int)(t % ch);
    vals_a[t] = (float)((double)fx[t] * scale[ch + k]);
    fx[t] = 0;  // ready for the next filter call: the accumulators are never cleared by a fill
    if (t < ch) vals_b[t] = 0.f;
}

// ---- order-preserving splat ------------------------------------------------------------------------------------------
// The reference splats sequentially (permutohedral.cpp:491-500 / :548-556): points in order, per point its d + 1
// vertices, `values[o] += w * in[i]` in float32 - a vertex' value is ONE chain of float additions in point order, and a
// different order gives different float32 bits.  The atomic splats above accumulate in arrival order: run-to-run
// noise of ~1e-7 relative that the lattice amplifies from EM iteration to EM iteration (cell assignment is discontinuous
// in sigma).  Here every vertex' chain is evaluated in the reference's order: the incidences of the splatted points are
// sorted by vertex id with a STABLE sort from an input written in the reference's point order (lat_segments); per filter
// call the terms are gathered into that order (k_seg_gather) and every chain is added up term by term by one thread
// (k_segchain_thread) or, when it is long, by one wave that keeps several hundred terms in flight (k_segchain_wave) - bit
// for bit the reference's float32 values, the same in every run.
__global__ __launch_bounds__(kBlock) void k_seg_keys(const int* __restrict__ offset, const int* __restrict__ ref_pos,
                                                     int64_t first, int64_t n_inc, int d1, unsigned* __restrict__ keys,
                                                     int* __restrict__ vals, int* __restrict__ seg, int64_t seg_elems) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t z = t; z < seg_elems; z += (int64_t)gridDim.x * kBlock) seg[z] = 0;  // vertices nobody splats into: empty
    if (t >= n_inc) return;
    const int64_t j = t / d1;
    const int r = (int)(t % d1);
    const int64_t p = first + (ref_pos ? (int64_t)ref_pos[j] : j);
    const int64_t inc = p * d1 + r;
    keys[t] = (unsigned)offset[inc];
    vals[t] = (int)inc;
}

__global__ __launch_bounds__(kBlock) void k_seg_bounds(const unsigned* __restrict__ keys, int64_t n_inc, int size,
                                                       int* __restrict__ seg) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_inc) return;
    const unsigned k = keys[t];
    if (t == 0 || keys[t - 1] != k) seg[k] = (int)t;
    if (t + 1 == n_inc || keys[t + 1] != k) seg[size + k] = (int)(t + 1);
}

// Pass 1 of a filter call: the terms `w * in[i]` (permutohedral.cpp:497 / :555, one float multiplication) of every
// incidence in SORTED order, one plane per channel: prod[k * stride + t].  Fully parallel - this is where the scattered
// reads happen; the chains below then stream contiguous memory.
__global__ __launch_bounds__(kBlock) void k_seg_gather(const int* __restrict__ sinc, const float* __restrict__ bary,
                                                       const float* __restrict__ in, int64_t n_inc, int d1, int ch,
                                                       float* __restrict__ prod, int64_t stride,
                                                       int* __restrict__ long_count) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t == 0) *long_count = 0;  // (list of the long chains, filled by k_segchain_thread of this filter call)
    if (t >= n_inc) return;
    const int inc = sinc[t];
    const float w = bary[inc];
    const float* __restrict__ row = in + (int64_t)(inc / d1) * ch;
    for (int k = 0; k < ch; ++k) prod[k * stride + t] = __fmul_rn(w, row[k]);
}

// Pass 2a: one thread per vertex adds its chain up, term by term, in order.  Chains longer than kLongSeg are left to
// k_segchain_wave (their vertices are appended to `long_list`).  vals_a / vals_b: the two value planes [(size + 1)][ch];
// row 0 (the "no neighbour" row of the blur) is zeroed in both, every other row of plane a is WRITTEN by whoever owns the
// vertex - nothing is cleared beforehand.
constexpr int kLongSeg = 64;
__global__ __launch_bounds__(kBlock) void k_segchain_thread(const int* __restrict__ seg, const float* __restrict__ prod,
                                                            int64_t stride, int ch, int size, float* __restrict__ vals_a,
                                                            float* __restrict__ vals_b, int* __restrict__ long_list,
                                                            int* __restrict__ long_count) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < ch) {
        vals_a[threadIdx.x] = 0.f;
        vals_b[threadIdx.x] = 0.f;
    }
    if (v >= size) return;
    const int start = seg[v], end = seg[size + v];
    if (end - start > kLongSeg) {
        long_list[atomicAdd(long_count, 1)] = (int)v;  // (the order of the list is irrelevant: one wave per entry)
        return;
    }
    float acc[kSplatMaxCh];
#pragma unroll
    for (int k = 0; k < kSplatMaxCh; ++k) acc[k] = 0.f;
    // eight terms per channel are fetched before any of them is added: the loads do not depend on the sums, only the
    // additions form a chain
    for (int t0 = start; t0 < end; t0 += 8) {
        float q[8][kSplatMaxCh];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int k = 0; k < kSplatMaxCh; ++k) q[j][k] = (k < ch && t0 + j < end) ? prod[k * stride + t0 + j] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (t0 + j < end)
#pragma unroll
                for (int k = 0; k < kSplatMaxCh; ++k) acc[k] = __fadd_rn(acc[k], q[j][k]);
    }
#pragma unroll
    for (int k = 0; k < kSplatMaxCh; ++k)
        if (k < ch) vals_a[(v + 1) * ch + k] = acc[k];
}

// Pass 2b: one wave per long chain (while the lattice has a few hundred vertices each collects ~10^4 terms).  All 64 lanes
// fetch - 64 consecutive terms per channel and round, kRing rounds in flight -, lane k < ch adds channel k's terms up in
// order out of LDS.  The chain itself is what bounds it: one dependent float addition per term.
constexpr int kRing = 8;
__global__ __launch_bounds__(kBlock) void k_segchain_wave(const int* __restrict__ seg, const float* __restrict__ prod,
                                                          int64_t stride, int ch, int size, float* __restrict__ vals_a,
                                                          const int* __restrict__ long_list,
                                                          const int* __restrict__ long_count) {
    __shared__ __attribute__((aligned(16))) float stage[kBlock / 64][kSplatMaxCh][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + wv;
    if (w >= *long_count) return;
    const int v = long_list[w];
    const int start = seg[v], end = seg[size + v];
    float pr[kRing][kSplatMaxCh];
    auto issue = [&](int slot, int base) {
#pragma unroll
        for (int k = 0; k < kSplatMaxCh; ++k) pr[slot][k] = (k < ch && base + lane < end) ? prod[k * stride + base + lane] : 0.f;
    };
#pragma unroll
    for (int s = 0; s < kRing; ++s) issue(s, start + 64 * s);
    float acc = 0.f;
    float (*lds)[64] = stage[wv];
    for (int base = start; base < end; base += 64 * kRing) {
#pragma unroll
        for (int s = 0; s < kRing; ++s) {
            const int b = base + 64 * s;
            if (b < end) {  // wave-uniform
#pragma unroll
                for (int k = 0; k < kSplatMaxCh; ++k)
                    if (k < ch) lds[k][lane] = pr[s][k];
                issue(s, b + 64 * kRing);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // LDS is in order within a wave: compiler ordering only
                const int cnt = end - b < 64 ? end - b : 64;
                if (lane < ch) {
                    const float* __restrict__ c = lds[lane];
                    if (cnt == 64) {
#pragma unroll
                        for (int j = 0; j < 64; j += 4) {
                            const float4 q = *reinterpret_cast<const float4*>(c + j);
                            acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, q.x), q.y), q.z), q.w);
                        }
                    } else {
                        for (int j = 0; j < cnt; ++j) acc = __fadd_rn(acc, c[j]);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    }
    if (lane < ch) vals_a[(int64_t)(v + 1) * ch + lane] = acc;
}

// seq_mask bit k set: channel k follows seqCompute (0.5*(n1+n2) evaluated in double, :510), else sseCompute.
__global__ __launch_bounds__(kBlock) void k_blur(const float* __restrict__ old, float* __restrict__ nw,
                                                 const int* __restrict__ nb1, const int* __restrict__ nb2, int size,
                                                 int ch, unsigned seq_mask) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)size * ch) return;
    const int v = (int)(t / ch), k = (int)(t % ch);
    const float a = old[(int64_t)(nb1[v] + 1) * ch + k], b = old[(int64_t)(nb2[v] + 1) * ch + k];
    const float o = old[(int64_t)(v + 1) * ch + k];
    const float s = __fadd_rn(a, b);
    float r;
    if ((seq_mask >> k) & 1u)
        r = (float)((double)o + 0.5 * (double)s);
    else
        r = __fadd_rn(o, __fmul_rn(0.5f, s));
    nw[(int64_t)(v + 1) * ch + k] = r;
}

__global__ __launch_bounds__(kBlock) void k_slice(const int* __restrict__ offset, const float* __restrict__ bary,
                                                  const float* __restrict__ vals, int64_t n_out, int d1, int ch,
                                                  float alpha, unsigned seq_mask, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_out * ch) return;
    const int64_t i = t / ch;
    const int k = (int)(t % ch);
    float acc = 0.f;
    for (int r = 0; r < d1; ++r) {
        const int o = offset[i * d1 + r] + 1;
        const float w = bary[i * d1 + r];
        const float v = vals[(int64_t)o * ch + k];
        if ((seq_mask >> k) & 1u)
            acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(w, v), alpha));   // (:526) w * value * alpha
        else
            acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(w, alpha), v));   // (:588-590) (w*alpha) * value
    }
    out[t] = acc;
}

}  // namespace

namespace prg {

// capacity for a buffer that has to hold `need` elements now and at most `worst` ever: four times the need, at least 4M
// elements, never more than the worst case - the lattice of an EM registration grows every iteration, and every
// reallocation (hipFree synchronises the device) is a bubble in the stream
static int64_t lat_grow(int64_t need, int64_t worst) {
    return std::max<int64_t>(need, std::min<int64_t>(worst, std::max<int64_t>(4 * need, (int64_t)1 << 22)));
}

// scale_factor[i] = float(1/sqrt((i+2)(i+1)) * inv_std_dev), inv_std_dev a float (permutohedral.cpp:180-183); zero from d on
static void lat_scale(int d, int with_blur, float* sc, int count) {
    const int d1 = d + 1;
    const float inv_std = with_blur ? (float)(sqrt(2.0 / 3.0) * d1) : (float)(sqrt(1.0 / 6.0) * d1);
    for (int i = 0; i < count; ++i) sc[i] = i < d ? (float)(1.0 / sqrt((double)((i + 2) * (i + 1))) * (double)inv_std) : 0.f;
}

// every how-many-th point creates the vertices in stage 1 of a build (the others look them up in stage 2); PRG_EMBED_PERIOD for A/B runs
static int embed_period() {
    static const int p = getenv("PRG_EMBED_PERIOD") ? std::max(2, std::min(64, atoi(getenv("PRG_EMBED_PERIOD")))) : 16;
    return p;
}

// Embedding launch over points [first, last) into `table`; side (tkeys may be null): the same points also go, with the
// scale factors ssc, into the side table of the speculative with_blur decision.
static void launch_embed(Lattice* L, int d, int64_t first, int64_t last, const float (&sc)[3], const EmbedTable& table,
                         const EmbedTable& side, const float (&ssc)[3], int sample = 0) {
    // sample 1 / 2: first must be 0; the every-16th sample has ceil(last / 16) points, the complement the rest
    const int period = embed_period();
    const int64_t count = sample == 0 ? last - first : (sample == 1 ? prg::ceil_div(last, period) : last - prg::ceil_div(last, period));
    if (sample) sample |= period << 2;
    const unsigned nb = (unsigned)prg::ceil_div(count, kBlock);
    if (nb == 0) return;
    hipStream_t st = L->stream;
    const FrFeat none = {nullptr, nullptr, nullptr, nullptr, 0, 0};
#define PRG_EMBED(DD)                                                                                              \
    if (L->prod)                                                                                                    \
        k_embed<DD, true><<<nb, kBlock, 0, st>>>(nullptr, *L->prod, first, last, sc[0], sc[1], sc[2], table,        \
                                                 L->pslot.p, L->bary.p, side, ssc[0], ssc[1], ssc[2], sample);      \
    else                                                                                                            \
        k_embed<DD, false><<<nb, kBlock, 0, st>>>(L->feat.p, none, first, last, sc[0], sc[1], sc[2], table,         \
                                                  L->pslot.p, L->bary.p, side, ssc[0], ssc[1], ssc[2], sample)
    if (d == 1) { PRG_EMBED(1); }
    else if (d == 2) { PRG_EMBED(2); }
    else { PRG_EMBED(3); }
#undef PRG_EMBED
}

// next generation of a table (see Lattice::gen): wraps by zeroing the table once every 65535 builds
static int next_generation(unsigned long long* table, int64_t cap, unsigned* gen, hipStream_t st) {
    if (*gen >= 0xFFFFu) {
        PRG_HIP(hipMemsetAsync(table, 0, cap * sizeof(unsigned long long), st));
        *gen = 0;
    }
    ++*gen;
    return PRG_OK;
}

// The five build buffers (see Lattice).  A build reuses them when they were created for the same d and hold its n points;
// a change of d re-creates them whatever their size, because the table's entry format follows d: (generation << 48) | key for
// d <= 3, a 64-bit hash in a table filled with 0xFF for d > 3.
static bool lat_build_fits(const Lattice* L, int64_t n, int d) { return d == L->d && n * (d + 1) <= L->pslot.cap; }

static void lat_release_build(Lattice* L) {
    L->tkeys.release(); L->slot_id.release(); L->pslot.release(); L->bary.release(); L->dkeys.release();
    L->d = 0;
}

// All five are released before the first is allocated (the peak stays one set), each exactly for n; a failure leaves all
// five empty, so the next build starts over.
static hipError_t lat_alloc_build(Lattice* L, int64_t n, int d) {
    const int d1 = d + 1;
    int64_t cap = 1;
    while (cap < 2 * n * d1) cap <<= 1;
    lat_release_build(L);
    hipError_t e = L->tkeys.reset(cap);
    if (e == hipSuccess) e = L->slot_id.reset(cap);
    if (e == hipSuccess) e = L->pslot.reset(n * d1);
    if (e == hipSuccess) e = L->bary.reset(n * d1);
    if (e == hipSuccess) e = L->dkeys.reset(n * d1);
    if (e == hipSuccess) L->d = d;
    else lat_release_build(L);
    return e;
}

// Feature lattices (3 < d <= 64): the structure of lat_build with the hashed-key kernels above.  Synchronises.
static int lat_build_generic(Lattice* L, int64_t n, int d, int with_blur) {
    const int d1 = d + 1;
    hipStream_t st = L->stream;
    if (!lat_build_fits(L, n, d)) {
        PRG_HIP(lat_alloc_build(L, n, d));
        L->prev_size[0] = L->prev_size[1] = 0;
    }
    PRG_HIP(L->count.ensure(2, 2));
    if (d != L->g_d) {
        L->rem0s.release();
        L->rank8.release();
        L->g_d = d;
    }
    PRG_HIP(L->rem0s.ensure(n * d1, n * d1));
    PRG_HIP(L->rank8.ensure(n * d1, n * d1));
    PRG_HIP(L->scale_dev.ensure(kMaxDG, kMaxDG));
    PRG_HIP(L->pinned.ensure(64, hipHostMallocDefault));
    L->n = n;
    L->with_blur = with_blur;
    float sc[kMaxDG];
    lat_scale(d, with_blur, sc, kMaxDG);
    PRG_HIP(hipMemcpyAsync(L->scale_dev.p, sc, sizeof(sc), hipMemcpyHostToDevice, st));
    PRG_HIP(hipStreamSynchronize(st));  // (sc lives on this stack frame)
    volatile int* host = reinterpret_cast<volatile int*>(L->pinned.p);
    int* count = L->count.p;
    L->built = false;
    L->seg_valid = false;
    for (int attempt = 0; attempt < 4; ++attempt) {
        const unsigned long long seed = 0x9e3779b97f4a7c15ull * (2 * attempt + 1), seed2 = 0xc2b2ae3d27d4eb4full * (2 * attempt + 3);
        const int64_t capu = L->tkeys.cap;
        L->cap_used = capu;
        const unsigned long long mask = (unsigned long long)capu - 1;
        PRG_HIP(hipMemsetAsync(L->tkeys.p, 0xFF, capu * sizeof(unsigned long long), st));
        PRG_HIP(hipMemsetAsync(count, 0, 2 * sizeof(int), st));
        L->count_clean = false;
        k_embed_g<<<(unsigned)prg::ceil_div(n, kBlock), kBlock, 0, st>>>(L->feat.p, n, d, L->scale_dev.p, L->tkeys.p, mask, seed,
                                                                         L->pslot.p, L->bary.p, L->rem0s.p, L->rank8.p, count + 1);
        k_compact<<<(unsigned)prg::ceil_div(capu, kBlock), kBlock, 0, st>>>(L->tkeys.p, capu, L->slot_id.p, L->dkeys.p, count);
        PRG_HIP(hipGetLastError());
        PRG_HIP(hipMemcpyAsync(L->pinned.p, count, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        PRG_HIP(hipStreamSynchronize(st));
        PRG_REQUIRE(host[1] == 0, PRG_ERR_STATE, "permutohedral lattice: hash table overflow at full capacity");
        L->size = host[0];
        const int64_t want = (int64_t)L->size + L->size / 4 + 1024;
        PRG_HIP(L->kfull.ensure((int64_t)L->size * d, want * d));
        PRG_HIP(L->gcheck.ensure(L->size, want));
        k_resolve<<<(unsigned)prg::ceil_div(prg::ceil_div(n * d1, 4), kBlock), kBlock, 0, st>>>(L->pslot.p, n * d1, L->slot_id.p, nullptr, nullptr, nullptr, 0u);
        PRG_HIP(hipMemsetAsync(L->gcheck.p, 0, (size_t)L->size * sizeof(unsigned long long), st));
        PRG_HIP(hipMemsetAsync(count + 1, 0, sizeof(int), st));  // now the collision flag
        k_store_keys_g<<<(unsigned)prg::ceil_div(n * d1, kBlock), kBlock, 0, st>>>(L->pslot.p, n, d, L->rem0s.p, L->rank8.p, seed2,
                                                                                  L->kfull.p, L->gcheck.p, count + 1);
        if (with_blur) {
            const int64_t need = 2 * (int64_t)d1 * L->size;
            PRG_HIP(L->nb.ensure(need, need));
            k_neighbours_g<<<(unsigned)prg::ceil_div((int64_t)L->size * d1, kBlock), kBlock, 0, st>>>(
                L->kfull.p, L->size, d, L->tkeys.p, mask, L->slot_id.p, L->gcheck.p, seed, seed2, L->nb.p,
                L->nb.p + (int64_t)d1 * L->size, count + 1);
        }
        PRG_HIP(hipGetLastError());
        PRG_HIP(hipMemcpyAsync(L->pinned.p, count, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        PRG_HIP(hipStreamSynchronize(st));
        if (host[1] == 0) {
            L->built = true;
            return PRG_OK;
        }
        // two different keys shared a 64-bit table hash (probability ~1e-7 per build): other seeds, again
    }
    prg::set_error("permutohedral lattice: key hash collisions persisted over 4 seeds");
    return PRG_ERR_STATE;
}

int lat_build(Lattice* L, int64_t n, int d, int with_blur, int64_t decide_above) {
    PRG_REQUIRE(d >= 1 && d <= kMaxDG, PRG_ERR_INVALID, "permutohedral lattice: feature dimension %d not in [1, %d]", d,
                kMaxDG);
    if (d > kMaxD) return lat_build_generic(L, n, d, with_blur);
    const int d1 = d + 1;
    hipStream_t st = L->stream;
    if (!lat_build_fits(L, n, d)) {
        PRG_HIP(lat_alloc_build(L, n, d));
        L->gen = 0;  // (generation 0 = zeroed memory: without the fill the table must not survive)
        const hipError_t e = hipMemsetAsync(L->tkeys.p, 0, L->tkeys.cap * sizeof(unsigned long long), st);
        if (e != hipSuccess) lat_release_build(L);
        PRG_HIP(e);
    }
    PRG_HIP(L->count.ensure(2, 2));
    PRG_HIP(L->pinned.ensure(64, hipHostMallocDefault));
    PRG_HIP(L->mail.ensure(1, hipHostMallocMapped | hipHostMallocCoherent));
    L->n = n;
    L->with_blur = with_blur;
    float sc[3];
    lat_scale(d, with_blur, sc, 3);
    // The table is sized from the previous lattice of the same kind (x8..16 head room: the lattice at most doubles
    // per EM iteration) so that the probes stay inside a few cache lines' worth of slots; an overflow falls back to the
    // worst-case size.  Nothing is cleared: the build takes the next generation of the table.
    const int mode = with_blur ? 1 : 0;
    const int64_t cap = L->tkeys.cap;
    int64_t capu = cap;
    if (L->prev_size[mode] > 0) {
        capu = 65536;
        while (capu < 8 * (int64_t)L->prev_size[mode]) capu <<= 1;
        if (capu > cap) capu = cap;
    }
    L->built = false;
    L->seg_valid = false;
    for (int attempt = 0; attempt < 2; ++attempt) {
        L->cap_used = capu;
        L->attempts = attempt + 1;
        PRG_TRY(next_generation(L->tkeys.p, cap, &L->gen, st));
        if (!L->count_clean) PRG_HIP(hipMemsetAsync(L->count.p, 0, 2 * sizeof(int), st));  // (normally left clean by k_resolve)
        L->count_clean = false;
        const unsigned long long mask = (unsigned long long)capu - 1;
        const EmbedTable main_table = {L->tkeys.p, mask, L->gen, L->count.p, L->slot_id.p, L->dkeys.p};
        const EmbedTable no_side = {nullptr, 0, 0, nullptr, nullptr, nullptr};
        const float no_sc[3] = {0.f, 0.f, 0.f};
        // stage 1 = every 16th point, stage 2 = the others, stage 0 = all points in one launch
        auto embed_stage = [&](int stage, const EmbedTable& side_table, const float (&side_sc)[3]) {
            launch_embed(L, d, 0, n, sc, main_table, side_table, side_sc, stage);
        };
        int host[2] = {0, 0};
        int64_t done = 0;
        if (decide_above >= 0 && n >= 4096) {  // stage 1: a sixteenth of the points; the vertex counter tells
            done = n / 16;
            embed_stage(1, no_side, no_sc);
            PRG_HIP(hipGetLastError());
            PRG_HIP(hipMemcpyAsync(L->pinned.p, L->count.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
            PRG_HIP(hipStreamSynchronize(st));
            host[0] = reinterpret_cast<volatile int*>(L->pinned.p)[0];
            host[1] = reinterpret_cast<volatile int*>(L->pinned.p)[1];
            if (host[1] == 0 && host[0] > decide_above) {
                L->size = host[0];
                if (getenv("PRG_DEBUG_LATTICE"))
                    fprintf(stderr, "[lattice] decision after %lld of %lld points: >= %d vertices > %lld (blur %d)\n",
                            (long long)done, (long long)n, host[0], (long long)decide_above, with_blur);
                return PRG_OK;  // prev_size[mode] keeps the last full count
            }
        } else if (n >= 4096) {
            // no decision to take, but the table is still filled in two launches: the first sixteenth of the points
            // creates most vertices almost uncontended, the rest then find them with plain reads - one launch over
            // all points has every wave compare-and-swap the same few hundred empty slots at once (3x slower while
            // the lattice is small; [r4] once it has tens of thousands of vertices a single launch is neither faster nor
            // slower - measured at C4 with the switch at 8k / 32k / 128k vertices: 4855 / 4864 / 4871 / 4885 it/s - so the
            // two stages stay unconditional)
            done = n / 16;
            if (L->side_fuse) {  // the prepared side stage (lat_side_stage) covers exactly these points: one launch for both
                float bsc[3];
                lat_scale(d, 1, bsc, 3);
                const EmbedTable side = {L->tkeys2.p, (unsigned long long)L->tkeys2.cap - 1, L->gen2, L->count2.p, nullptr, nullptr};
                embed_stage(1, side, bsc);
                L->side_fuse = false;
                L->side_pending = true;
            } else {
                embed_stage(1, no_side, no_sc);
            }
        }
        if (host[1] == 0) {
            embed_stage(done > 0 ? 2 : 0, no_side, no_sc);
            // the resolve pass goes out right behind the embedding and tells the host the counters while it runs: no
            // device-to-host copy, no stream synchronisation, the queue does not drain (on an overflow - rare - it has
            // resolved garbage, which the retry overwrites)
            const unsigned seq = ++L->mail_seq;
            k_resolve<<<(unsigned)prg::ceil_div(prg::ceil_div(n * d1, 4), kBlock), kBlock, 0, st>>>(L->pslot.p, n * d1, L->slot_id.p, L->count.p,
                                                                                 L->side_pending ? L->count2.p : nullptr,
                                                                                 L->mail.dev, seq);
            PRG_HIP(hipGetLastError());
            volatile LatticeMail* mb = L->mail.p;
            {
                hipError_t werr;
                const bool got = prg::wait_mailbox(&mb->seq, seq, st, &werr);
                PRG_HIP(werr);
                PRG_REQUIRE(got, PRG_ERR_HIP, "permutohedral lattice: the vertex count never reached the host");
            }
            host[0] = mb->size;
            host[1] = mb->overflow;
            L->count_clean = true;
            if (L->side_pending) {
                L->side_size = mb->side_size;
                L->side_overflow = mb->side_overflow;
                L->side_pending = false;
                L->count2_clean = true;
            }
        }
        L->size = host[0];
        if (getenv("PRG_DEBUG_LATTICE"))
            fprintf(stderr, "[lattice] attempt %d capu %lld prev %d size %d overflow %d blur %d\n", attempt, (long long)capu,
                    L->prev_size[mode], L->size, host[1], with_blur);
        if (host[1] == 0 && (int64_t)L->size * 2 <= capu) break;
        PRG_REQUIRE(capu < cap, PRG_ERR_STATE, "permutohedral lattice: hash table overflow at full capacity");
        capu = cap;
    }
    L->built = true;
    L->prev_size[mode] = L->size;
    const unsigned long long mask = (unsigned long long)L->cap_used - 1;  // (k_resolve is already in the queue)
    if (with_blur) {
        // (generous: the lattice grows from iteration to iteration and hipFree / hipMalloc drain the device)
        const int64_t need = 2 * (int64_t)d1 * L->size;
        PRG_HIP(L->nb.ensure(need, lat_grow(need, 2 * (int64_t)d1 * n * d1)));
        int* nb1 = L->nb.p;
        int* nb2 = L->nb.p + (int64_t)d1 * L->size;
        const unsigned g = (unsigned)prg::ceil_div((int64_t)L->size * d1, kBlock);
        if (d == 1) k_neighbours<1><<<g, kBlock, 0, st>>>(L->dkeys.p, L->size, L->tkeys.p, mask, L->slot_id.p, nb1, nb2, L->gen);
        else if (d == 2) k_neighbours<2><<<g, kBlock, 0, st>>>(L->dkeys.p, L->size, L->tkeys.p, mask, L->slot_id.p, nb1, nb2, L->gen);
        else k_neighbours<3><<<g, kBlock, 0, st>>>(L->dkeys.p, L->size, L->tkeys.p, mask, L->slot_id.p, nb1, nb2, L->gen);
        PRG_HIP(hipGetLastError());
    }
    return PRG_OK;
}

int lat_side_stage(Lattice* L, int64_t n, int d) {
    const int d1 = d + 1;
    hipStream_t st = L->stream;
    const int64_t n16 = prg::ceil_div(n, embed_period());
    int64_t want = 1;
    while (want < 4 * n16 * d1) want <<= 1;
    bool grown;
    PRG_HIP(L->tkeys2.ensure(want, want, &grown));
    if (grown) {
        L->gen2 = 0;
        const hipError_t e = hipMemsetAsync(L->tkeys2.p, 0, want * sizeof(unsigned long long), st);
        if (e != hipSuccess) L->tkeys2.release();
        PRG_HIP(e);
    }
    PRG_HIP(L->count2.ensure(2, 2));
    PRG_HIP(L->pinned.ensure(64, hipHostMallocDefault));
    PRG_TRY(next_generation(L->tkeys2.p, L->tkeys2.cap, &L->gen2, st));
    if (!L->count2_clean) PRG_HIP(hipMemsetAsync(L->count2.p, 0, 2 * sizeof(int), st));
    L->count2_clean = false;
    L->side_fuse = true;  // launched by the next lat_build on this lattice, together with its first sixteenth
    return PRG_OK;
}

// How the splat accumulates (prg_lattice_set_splat_mode; process-wide):
//   0  float atomics in arrival order (round-off level run-to-run noise; measurement baseline)
//   1  fixed-point atomics (default): order-independent - the same bits in every run, each vertex the correctly rounded exact sum
//   2  the reference's own order: every vertex one sequential float32 chain in point order - the reference's bits
//      (permutohedral.cpp:491-500); costs a sort of the incidences per lattice and a strictly sequential chain per vertex
static int g_splat_mode = []() {
    const char* e = getenv("PRG_SPLAT_MODE");
    const int m = e ? atoi(e) : 1;
    return m < 0 || m > 2 ? 1 : m;
}();

// Sorted incidence lists of the current lattice for the points >= first (once per lattice build; every filter call on the
// lattice reuses them).  No synchronisation.
static int lat_segments(Lattice* L, int64_t first) {
    if (L->seg_valid && L->seg_first == first) return PRG_OK;
    const int d1 = L->d + 1;
    hipStream_t st = L->stream;
    const int64_t n_inc = (L->n - first) * d1;
    PRG_REQUIRE(n_inc > 0 && n_inc < (int64_t)1 << 31 && L->n * d1 < (int64_t)1 << 31, PRG_ERR_INVALID,
                "permutohedral lattice: too many point-vertex incidences for the ordered splat");
    PRG_HIP(L->skeys.ensure(2 * n_inc, 2 * n_inc));
    PRG_HIP(L->svals.ensure(2 * n_inc, 2 * n_inc));
    const int64_t want = (int64_t)L->size + L->size / 4 + 1024;
    PRG_HIP(L->seg.ensure(2 * (int64_t)L->size, 2 * want));
    unsigned* skeys_out = L->skeys.p + L->skeys.cap / 2;  // (each array's second half: the sort's output)
    int* svals_out = L->svals.p + L->svals.cap / 2;
    unsigned bits = 1;
    while (((int64_t)1 << bits) < (int64_t)L->size) ++bits;
    size_t need = 0;
    PRG_TRY(prg::sort_pairs_u32(nullptr, &need, L->skeys.p, skeys_out, L->svals.p, svals_out, (unsigned)n_inc, bits, st));
    PRG_HIP(L->sort_tmp.ensure((int64_t)need, (int64_t)(need + (need >> 2) + 256)));
    const unsigned g = (unsigned)prg::ceil_div(n_inc, kBlock);
    k_seg_keys<<<g, kBlock, 0, st>>>(L->pslot.p, L->ref_pos, first, n_inc, d1, L->skeys.p, L->svals.p, L->seg.p, 2 * (int64_t)L->size);
    size_t bytes = (size_t)L->sort_tmp.cap;
    PRG_TRY(prg::sort_pairs_u32(L->sort_tmp.p, &bytes, L->skeys.p, skeys_out, L->svals.p, svals_out, (unsigned)n_inc, bits, st));
    k_seg_bounds<<<g, kBlock, 0, st>>>(skeys_out, n_inc, L->size, L->seg.p);
    PRG_HIP(hipGetLastError());
    L->seg_valid = true;
    L->seg_first = first;
    return PRG_OK;
}

int lat_slice(Lattice* L, const float* vals, float alpha, int ch, int64_t n_out, unsigned seq_mask, float* out) {
    k_slice<<<(unsigned)prg::ceil_div(n_out * ch, kBlock), kBlock, 0, L->stream>>>(L->pslot.p, L->bary.p, vals, n_out, L->d + 1, ch,
                                                                                  alpha, seq_mask, out);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

int lat_filter(Lattice* L, const float* in, int ch, int64_t first, int64_t n_out, unsigned seq_mask, float* out,
               bool defer_slice) {
    const int d1 = L->d + 1;
    hipStream_t st = L->stream;
    const int64_t plane = (int64_t)(L->size + 1) * ch;
    PRG_HIP(L->vals.ensure(2 * plane, lat_grow(2 * plane, 2 * (L->n * d1 + 1) * ch)));
    float* a = L->vals.p;
    float* b = L->vals.p + plane;
    const int* pslot = L->pslot.p;
    const float* bary = L->bary.p;
    if (g_splat_mode == 2 && ch <= kSplatMaxCh) {
        PRG_TRY(lat_segments(L, first));
        const int* sinc = L->svals.p + L->svals.cap / 2;
        const int64_t n_inc = (L->n - first) * d1;
        PRG_HIP(L->terms.ensure(n_inc * ch, n_inc * ch));
        const int64_t max_long = n_inc / (kLongSeg + 1) + 1;
        PRG_HIP(L->long_list.ensure(max_long + 1, max_long + 1));
        int* long_count = L->long_list.p + max_long;
        k_seg_gather<<<(unsigned)prg::ceil_div(n_inc, kBlock), kBlock, 0, st>>>(sinc, bary, in, n_inc, d1, ch, L->terms.p, n_inc,
                                                                               long_count);
        k_segchain_thread<<<(unsigned)prg::ceil_div(L->size, kBlock), kBlock, 0, st>>>(L->seg.p, L->terms.p, n_inc, ch, L->size, a, b,
                                                                                      L->long_list.p, long_count);
        k_segchain_wave<<<(unsigned)prg::ceil_div(max_long, kBlock / 64), kBlock, 0, st>>>(L->seg.p, L->terms.p, n_inc, ch, L->size, a,
                                                                                         L->long_list.p, long_count);
    } else if (g_splat_mode >= 1) {
        // fixed point: per-channel scale from the largest |value| (cached while the caller says the values have not changed)
        bool grown;
        PRG_HIP(L->fx_scale.ensure(2 * 32 + 32, 2 * 32 + 32, &grown));
        if (grown) L->fx_scale_key = nullptr;
        double* fx_scale = L->fx_scale.p;
        unsigned* maxabs = reinterpret_cast<unsigned*>(fx_scale + 64);
        if (L->fx_scale_key != in || L->fx_scale_ch != ch || !L->fx_scale_static) {
            PRG_HIP(hipMemsetAsync(maxabs, 0, 32 * sizeof(unsigned), st));
            const int64_t total = (L->n - first) * ch;
            const unsigned gm = (unsigned)std::min<int64_t>(prg::ceil_div(total, kBlock), 2048);
            k_chan_maxabs<<<gm, kBlock, 0, st>>>(in, first, L->n, ch, maxabs);
            k_chan_scale<<<1, 32, 0, st>>>(maxabs, ch, (double)(L->n - first), fx_scale);
            L->fx_scale_key = in;
            L->fx_scale_ch = ch;
        }
        PRG_HIP(L->fx.ensure(plane, lat_grow(plane, (L->n * d1 + 1) * ch), &grown));
        if (grown) {  // zeroed once: from here on k_fix_to_float keeps it zero
            const hipError_t e = hipMemsetAsync(L->fx.p, 0, (size_t)L->fx.cap * sizeof(long long), st);
            if (e != hipSuccess) L->fx.release();
            PRG_HIP(e);
        }
        long long* fx = L->fx.p;
        static const bool wide_table = !(getenv("PRG_SPLAT_TABLE") && atoi(getenv("PRG_SPLAT_TABLE")) == 0);
        if (ch <= 5 && wide_table)
            k_splat_lds<true, 9, 5><<<(unsigned)prg::ceil_div(L->n - first, kSplatPts), kBlock, 0, st>>>(
                pslot, bary, in, first, L->n, d1, ch, a, fx, fx_scale);
        else if (ch <= kSplatMaxCh)
            k_splat_lds<true, 8, 8><<<(unsigned)prg::ceil_div(L->n - first, kSplatPts), kBlock, 0, st>>>(
                pslot, bary, in, first, L->n, d1, ch, a, fx, fx_scale);
        else
            k_splat<true><<<(unsigned)prg::ceil_div((L->n - first) * d1, kBlock), kBlock, 0, st>>>(
                pslot, bary, in, first, L->n, d1, ch, a, fx, fx_scale);
        k_fix_to_float<<<(unsigned)prg::ceil_div(plane, kBlock), kBlock, 0, st>>>(fx, plane, ch, fx_scale, a, b);
    } else {
        PRG_HIP(hipMemsetAsync(a, 0, 2 * plane * sizeof(float), st));
        if (ch <= kSplatMaxCh)
            k_splat_lds<false, 8, 8><<<(unsigned)prg::ceil_div(L->n - first, kSplatPts), kBlock, 0, st>>>(
                pslot, bary, in, first, L->n, d1, ch, a, nullptr, nullptr);
        else
            k_splat<false><<<(unsigned)prg::ceil_div((L->n - first) * d1, kBlock), kBlock, 0, st>>>(
                pslot, bary, in, first, L->n, d1, ch, a, nullptr, nullptr);
    }
    if (L->with_blur) {
        const int* nb1 = L->nb.p;
        const int* nb2 = L->nb.p + (int64_t)d1 * L->size;
        for (int j = 0; j < d1; ++j) {
            k_blur<<<(unsigned)prg::ceil_div((int64_t)L->size * ch, kBlock), kBlock, 0, st>>>(
                a, b, nb1 + (int64_t)j * L->size, nb2 + (int64_t)j * L->size, L->size, ch, seq_mask);
            float* t = a; a = b; b = t;
        }
    }
    const float alpha = 1.0f / (1.0f + powf(2.0f, (float)-L->d));
    PRG_HIP(hipGetLastError());
    if (defer_slice) {
        L->pend_vals = a;
        L->pend_alpha = alpha;
        return PRG_OK;
    }
    return lat_slice(L, a, alpha, ch, n_out, seq_mask, out);
}

}  // namespace prg

struct prg_ph {
    prg::Lattice L;
    prg::Lattice& ctx() { return L; }  // device and stream (plan_base.h)
};

extern "C" {

int prg_lattice_set_splat_mode(int mode) {
    PRG_REQUIRE(mode >= 0 && mode <= 2, PRG_ERR_INVALID,
                "prg_lattice_set_splat_mode: mode must be 0 (float atomics), 1 (fixed-point atomics) or 2 (reference order)");
    prg::g_splat_mode = mode;
    return PRG_OK;
}

// ---------------------------------------------------------------------------------------------
// stand-alone lattice (gaussian_filtering.Permutohedral)
// ---------------------------------------------------------------------------------------------
int prg_ph_create(prg_ph** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_ph_destroy(prg_ph* h) {
    return prg::destroy_handle(h);  // (the lattice's buffers release themselves)
}

int prg_ph_init(prg_ph* h, const float* points_hd, int64_t n, int dim, int with_blur) {
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_ph_init: NULL argument");
    PRG_REQUIRE(n > 0 && dim >= 1 && dim <= kMaxDG, PRG_ERR_INVALID,
                "prg_ph_init: need n > 0 and feature dimension in [1, %d] (got n=%lld d=%d)", kMaxDG, (long long)n, dim);
    PRG_ENTER(h->L.device);
    prg::Lattice* L = &h->L;
    L->n = 0;  // "not initialised" until the build has gone through
    PRG_HIP(L->feat.reset(n * dim));
    PRG_HIP(hipMemcpyAsync(L->feat.p, points_hd, (size_t)n * dim * sizeof(float), hipMemcpyDefault, L->stream));
    const int st = prg::lat_build(L, n, dim, with_blur ? 1 : 0);
    if (st != PRG_OK) L->n = 0;
    return st;
}

int prg_ph_lattice_size(prg_ph* h, int* size) {
    PRG_REQUIRE(h && size, PRG_ERR_INVALID, "prg_ph_lattice_size: NULL argument");
    PRG_REQUIRE(h->L.n > 0, PRG_ERR_STATE, "prg_ph_lattice_size: lattice not initialised");
    *size = h->L.size;
    return PRG_OK;
}

int prg_ph_filter(prg_ph* h, const float* values_hd, int channels, float* out_hd) {
    PRG_REQUIRE(h && values_hd && out_hd, PRG_ERR_INVALID, "prg_ph_filter: NULL argument");
    PRG_REQUIRE(h->L.n > 0, PRG_ERR_STATE, "prg_ph_filter: lattice not initialised");
    PRG_REQUIRE(channels >= 1 && channels <= 32, PRG_ERR_INVALID, "prg_ph_filter: channels must be in [1, 32]");
    PRG_ENTER(h->L.device);
    prg::Lattice* L = &h->L;
    const int64_t count = L->n * channels;
    const size_t nb = (size_t)count * sizeof(float);
    PRG_HIP(L->io.ensure(2 * count, 2 * count));
    float* din = L->io.p;
    float* dout = L->io.p + count;
    PRG_HIP(hipMemcpyAsync(din, values_hd, nb, hipMemcpyDefault, L->stream));
    // <= 2 channels take the reference's seqCompute arithmetic, more take sseCompute (permutohedral.cpp:612-615)
    const unsigned seq_mask = channels <= 2 ? 0xFFFFFFFFu : 0u;
    PRG_TRY(prg::lat_filter(L, din, channels, 0, L->n, seq_mask, dout));
    PRG_HIP(hipMemcpyAsync(out_hd, dout, nb, hipMemcpyDefault, L->stream));
    PRG_HIP(hipStreamSynchronize(L->stream));
    return PRG_OK;
}

}  // extern "C"
