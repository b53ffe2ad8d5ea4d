// Particle inflow and outflow for gfx950 (build-defined: the reference's ParticleContextAdd / Remove are empty,
// Particle.c:120-130; model in include/dedflow.h).
//
// Outflow: flag -> exclusive scan of the keep flags (dfl_exclusive_scan_i32) -> one scatter pass that moves every piece of
// per-particle state to its new id.  Thread i owns particle i: it reads its own records and writes them to newid[i];
// its history row is copied entry by entry (live entries only), partner keys remapped through newid.  Stable, no atomics.
// Inflow: block (one thread per particle, integer atomics on the slot flags: order-independent) -> select (rank keys of
// the slots, one radix sort by (key, slot)) -> append (one thread per wanted slot).
//
// Bitwise parity with the numpy model (tests/flow_model.py) needs the exact operation order of include/dedflow.h: no
// fused multiply-add anywhere in this file.
#include "dfl_common.hpp"
#include <cstring>
#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;
constexpr uint64_t BLOCKED_KEY = 1ull << 63;

__device__ __forceinline__ uint64_t splitmix64(uint64_t a) {
    uint64_t z = a + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t slot_hash(const dfl_inlet& in, long long k, int axis) {
    return splitmix64(splitmix64(splitmix64(in.seed) ^ in.call) ^ (4ull * (uint64_t)k + (uint64_t)axis));
}

__device__ __forceinline__ double unit_pm1(uint64_t h) { return 2.0 * ((double)(h >> 11) * 0x1p-53) - 1.0; }

// candidate centre of slot k = i + nu j in this call
__device__ __forceinline__ void slot_centre(const dfl_inlet& in, int k, double c[3]) {
    const int i = k % in.nu, j = k / in.nu;
    const double r0 = unit_pm1(slot_hash(in, k, 0)), r1 = unit_pm1(slot_hash(in, k, 1));
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = (((in.base[d] + (double)i * in.pu[d]) + (double)j * in.pv[d]) + r0 * in.ou[d]) + r1 * in.ov[d];
}

__global__ __launch_bounds__(BLK) void flow_flag_kernel(I P, const T* __restrict__ coord, dfl_outflow_planes pl,
                                                       const I* __restrict__ tet, int by_tet, I* __restrict__ keep,
                                                       I* __restrict__ rtet) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const double x0 = coord[3 * (size_t)i], x1 = coord[3 * (size_t)i + 1], x2 = coord[3 * (size_t)i + 2];
    bool out = false;
    for (int k = 0; k < pl.num; ++k) out |= ((pl.plane[k][0] * x0 + pl.plane[k][1] * x1) + pl.plane[k][2] * x2) > pl.plane[k][3];
    const int t = tet ? tet[i] : 0;
    if (by_tet && t == -1) out = true;
    keep[i] = out ? 0 : 1;
    if (rtet) rtet[i] = out ? t : -1;
}

__device__ __forceinline__ void copy3(const T* __restrict__ s, T* __restrict__ d, size_t i, size_t j) {
    const double a = s[3 * i], b = s[3 * i + 1], c = s[3 * i + 2];
    d[3 * j] = a;
    d[3 * j + 1] = b;
    d[3 * j + 2] = c;
}

__global__ __launch_bounds__(BLK) void flow_compact_kernel(I P, const I* __restrict__ keep, const I* __restrict__ newid,
                                                          dfl_flow_fields f) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P || !keep[i]) return;
    const size_t j = (size_t)newid[i];
    int a = f.first[0];
    for (; a < f.first[1]; ++a) static_cast<I*>(f.pair[a].dst)[j] = static_cast<const I*>(f.pair[a].src)[i];
    for (; a < f.first[2]; ++a) static_cast<uint64_t*>(f.pair[a].dst)[j] = static_cast<const uint64_t*>(f.pair[a].src)[i];
    for (; a < f.first[3]; ++a) copy3(static_cast<const T*>(f.pair[a].src), static_cast<T*>(f.pair[a].dst), (size_t)i, j);
    for (; a < f.first[4]; ++a) {
        const double4 l = static_cast<const double4*>(f.pair[a].src)[i];
        static_cast<double4*>(f.pair[a].dst)[j] = l;
    }
    if (f.hrow_src) {
        const int n = f.hcount_src[i];
        const dfl_contact_hist* src = f.hrow_src + (size_t)i * DFL_DEM_MAX_HISTORY;
        dfl_contact_hist* dst = f.hrow_dst + j * DFL_DEM_MAX_HISTORY;
        int m = 0;
        for (int e = 0; e < n; ++e) {
            const ulonglong2 lo = reinterpret_cast<const ulonglong2*>(src + e)[0];  // key, xi[0]
            const double2 hi = reinterpret_cast<const double2*>(src + e)[1];        // xi[1], xi[2]
            uint64_t key = lo.x;
            if ((key >> 62) == 0) {  // partner particle
                const int p = (int)(key & 0x3fffffffffffffffull);
                if (!keep[p]) continue;
                key = (uint64_t)newid[p];
            }
            reinterpret_cast<ulonglong2*>(dst + m)[0] = make_ulonglong2(key, lo.y);
            reinterpret_cast<double2*>(dst + m)[1] = hi;
            ++m;
        }
        f.hcount_dst[j] = m;
    }
}

// radius of slot k in call c (polydisperse inflow): r_lo + (r_hi - r_lo) u, u = (H(c, k, 3) >> 11) 2^-53
__device__ __forceinline__ double slot_radius(const dfl_inlet& in, int k, double r_lo, double r_hi) {
    return r_lo + (r_hi - r_lo) * ((double)(slot_hash(in, k, 3) >> 11) * 0x1p-53);
}

// POLY: particle p has radius rad[p], the slots radii in [r_lo, r_hi]: the prefilter widths use r_p + r_hi in place of 2R
// and slot k is blocked when dist^2 < (r_p + r_k)^2
template <bool POLY>
__global__ __launch_bounds__(BLK) void inflow_block_kernel(I P, const T* __restrict__ coord, dfl_inlet in, T radius,
                                                          I* __restrict__ blocked, const T* __restrict__ rad, T r_lo, T r_hi) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= P) return;
    const double y[3] = {coord[3 * (size_t)p], coord[3 * (size_t)p + 1], coord[3 * (size_t)p + 2]};
    const double rel[3] = {y[0] - in.o[0], y[1] - in.o[1], y[2] - in.o[2]};
    const double ry = POLY ? rad[p] : 0.0;
    const double two_r = POLY ? ry + r_hi : 2.0 * radius;
    const double dn = (rel[0] * in.nrm[0] + rel[1] * in.nrm[1]) + rel[2] * in.nrm[2];
    if (!(fabs(dn) < two_r + in.plane_tol)) return;  // (a NaN centre blocks nothing)
    // conservative slot ranges along u and v (one extra slot per side against rounding); the exact test decides
    const double su = (rel[0] * in.uhat[0] + rel[1] * in.uhat[1]) + rel[2] * in.uhat[2];
    const double sv = (rel[0] * in.vhat[0] + rel[1] * in.vhat[1]) + rel[2] * in.vhat[2];
    const double wu = two_r + in.ju + in.plane_tol, wv = two_r + in.jv + in.plane_tol;
    const double ilo = floor((su - wu) / in.pitch_u - 0.5) - 1.0, ihi = floor((su + wu) / in.pitch_u - 0.5) + 1.0;
    const double jlo = floor((sv - wv) / in.pitch_v - 0.5) - 1.0, jhi = floor((sv + wv) / in.pitch_v - 0.5) + 1.0;
    if (ihi < 0.0 || jhi < 0.0 || ilo > (double)(in.nu - 1) || jlo > (double)(in.nv - 1)) return;
    const int i0 = ilo < 0.0 ? 0 : (int)ilo, i1 = ihi > (double)(in.nu - 1) ? in.nu - 1 : (int)ihi;
    const int j0 = jlo < 0.0 ? 0 : (int)jlo, j1 = jhi > (double)(in.nv - 1) ? in.nv - 1 : (int)jhi;
    const double lim = two_r * two_r;
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) {
            const int k = i + in.nu * j;
            double c[3];
            slot_centre(in, k, c);
            const double d0 = y[0] - c[0], d1 = y[1] - c[1], d2 = y[2] - c[2];
            double l = lim;
            if (POLY) {
                const double rr = ry + slot_radius(in, k, r_lo, r_hi);
                l = rr * rr;
            }
            if ((d0 * d0 + d1 * d1) + d2 * d2 < l) atomicOr(&blocked[k], 1);
        }
}

__global__ __launch_bounds__(BLK) void inflow_key_kernel(dfl_inlet in, I nslot, const I* __restrict__ blocked,
                                                        uint64_t* __restrict__ key, I* __restrict__ slot) {
    const int k = blockIdx.x * BLK + threadIdx.x;
    if (k >= nslot) return;
    key[k] = blocked[k] ? BLOCKED_KEY : slot_hash(in, k, 2) >> 1;
    slot[k] = k;
}

// POLY: also radius[i] = r_k and mass[i] = m0 ((q q) q), q = r_k / r0
template <bool POLY>
__global__ __launch_bounds__(BLK) void inflow_append_kernel(I P, I want, dfl_inlet in, const uint64_t* __restrict__ key,
                                                           const I* __restrict__ slot, int64_t first_tag, T* __restrict__ coord,
                                                           T* __restrict__ vel, T* __restrict__ acc, int64_t* __restrict__ tag,
                                                           T* __restrict__ omega, T* __restrict__ alpha, I* __restrict__ hist_count,
                                                           I* __restrict__ tet, T* __restrict__ lambda, T* __restrict__ imp,
                                                           I* __restrict__ count, T* __restrict__ radius, T* __restrict__ mass,
                                                           T r_lo, T r_hi, T r0, T m0) {
    const int k = blockIdx.x * BLK + threadIdx.x;
    if (k >= want) return;
    // the free slots sort first: the inserted ones are the prefix [0, n) of the first `want`
    const bool free_k = key[k] < BLOCKED_KEY;
    if (k == 0 && !free_k) *count = 0;
    if (!free_k) return;
    if (k + 1 == want || key[k + 1] >= BLOCKED_KEY) *count = k + 1;  // (want <= nslot)
    const size_t i = (size_t)P + k;
    double c[3];
    slot_centre(in, slot[k], c);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        coord[3 * i + d] = c[d];
        vel[3 * i + d] = in.vel[d];
        acc[3 * i + d] = 0.0;
        if (omega) omega[3 * i + d] = 0.0;
        if (alpha) alpha[3 * i + d] = 0.0;
        if (imp) imp[3 * i + d] = 0.0;
    }
    tag[i] = first_tag + k;
    if (POLY) {
        const double r = slot_radius(in, slot[k], r_lo, r_hi), q = r / r0;
        radius[i] = r;
        mass[i] = m0 * ((q * q) * q);
    }
    if (hist_count) hist_count[i] = 0;
    if (tet) {
        tet[i] = -1;
        reinterpret_cast<double4*>(lambda)[i] = make_double4(0.0, 0.0, 0.0, 0.0);
    }
}

}  // namespace

extern "C" {

void dfl_flow_flag(I P, const T* coord, dfl_outflow_planes planes, const I* tet, int by_tet, I* keep, I* rtet, void* stream) {
    if (P <= 0) return;
    flow_flag_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, coord, planes, tet, by_tet, keep, rtet);
    DFL_LAUNCH_CHECK();
}

void dfl_flow_compact(I P, const I* keep, const I* newid, dfl_flow_fields f, void* stream) {
    if (P <= 0) return;
    flow_compact_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, keep, newid, f);
    DFL_LAUNCH_CHECK();
}

void dfl_inflow_block(I P, const T* coord, dfl_inlet in, T radius, const T* radius_i, T r_lo, T r_hi, I* blocked, void* stream) {
    const long long nslot = (long long)in.nu * in.nv;
    if (nslot <= 0) return;
    DFL_GUARD(hipMemsetAsync(blocked, 0, (size_t)nslot * sizeof(I), S(stream)));
    if (P <= 0) return;
    if (radius_i)
        inflow_block_kernel<true><<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, coord, in, 0.0, blocked, radius_i, r_lo, r_hi);
    else
        inflow_block_kernel<false><<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, coord, in, radius, blocked, nullptr, 0.0, 0.0);
    DFL_LAUNCH_CHECK();
}

int64_t dfl_inflow_select_temp_bytes(I nslot) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const I*)nullptr, (I*)nullptr,
                                    (size_t)(nslot > 0 ? nslot : 1));
    return (int64_t)bytes + 16;
}

void dfl_inflow_select(dfl_inlet in, const I* blocked, uint64_t* key, uint64_t* key_out, I* slot, I* slot_out, void* temp,
                       int64_t temp_bytes, void* stream) {
    const I nslot = in.nu * in.nv;
    if (nslot <= 0) return;
    inflow_key_kernel<<<ceil_div(nslot, BLK), BLK, 0, S(stream)>>>(in, nslot, blocked, key, slot);
    DFL_LAUNCH_CHECK();
    size_t bytes = (size_t)temp_bytes;
    DFL_GUARD(rocprim::radix_sort_pairs(temp, bytes, key, key_out, slot, slot_out, (size_t)nslot, 0, 64, S(stream)));
}

void dfl_inflow_append(I P, I want, dfl_inlet in, const uint64_t* key_sorted, const I* slot_sorted, int64_t first_tag, T* coord,
                       T* vel, T* acc, int64_t* tag, T* omega, T* alpha, I* hist_count, I* tet, T* lambda, T* imp, T* radius_i,
                       T* mass_i, T r_lo, T r_hi, T r0, T m0, I* count, void* stream) {
    const I nslot = in.nu * in.nv;
    if (want > nslot) want = nslot;
    if (want <= 0) {
        DFL_GUARD(hipMemsetAsync(count, 0, sizeof(I), S(stream)));
        return;
    }
    if (radius_i)
        inflow_append_kernel<true><<<ceil_div(want, BLK), BLK, 0, S(stream)>>>(P, want, in, key_sorted, slot_sorted, first_tag,
                                                                              coord, vel, acc, tag, omega, alpha, hist_count, tet,
                                                                              lambda, imp, count, radius_i, mass_i, r_lo, r_hi, r0,
                                                                              m0);
    else
        inflow_append_kernel<false><<<ceil_div(want, BLK), BLK, 0, S(stream)>>>(P, want, in, key_sorted, slot_sorted, first_tag,
                                                                               coord, vel, acc, tag, omega, alpha, hist_count, tet,
                                                                               lambda, imp, count, nullptr, nullptr, 0.0, 0.0, 1.0,
                                                                               1.0);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
