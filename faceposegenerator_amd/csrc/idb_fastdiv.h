// Division of a 32-bit numerator by a launch constant without a divide: the host turns the divisor into {mul, add, sh} once per
// launch, the device computes  q = (mulhi(n, mul) + (n & add)) >> sh  — four VALU/SALU instructions where v_rcp_iflag_f32 + Newton
// steps + fix-ups were 25-40 (and 100+ for a 64-bit numerator).  Plain C++ on the host (no HIP headers needed), so the arithmetic is
// tested without a GPU (tests/test_fastdiv_cpu.py).
//
// Three shapes of {mul, add, sh}, one device expression:
//   * power of two d = 2^k:                        {0, ~0, k}                    q = n >> k                 (d = 1: k = 0)
//   * ONE multiply-high, r = ceil(2^32 / d):       {r, 0, 0}                     q = mulhi(n, r)
//     exact for every n <= nmax iff idb_fastdiv_mulhi_exact(d, nmax); with e = r d - 2^32 (0 < e < d) the quotient of n = k d + j is
//     one too large iff n e >= 2^32 (d - j), first for j = d - 1 (d <= 2^16: the thresholds of the other residues lie >= d beyond it)
//   * fallback, the round-up method of Granlund & Montgomery with a 33-bit multiplier 2^32 + m, l = ceil(log2 d),
//     m = floor(2^32 (2^l - d) / d) + 1:           {m, ~0, l}                    q = (mulhi(n, m) + n) >> l
//     exact for every 32-bit n as long as the sum does not wrap: mulhi(n, m) < n, so n < 2^31 is enough.
// idb_fastdiv_make picks the first shape that is exact on [0, nmax]; nmax < 2^31 is the range the GEMM host code admits (M, tile
// index and kz * ktiles are all checked < 2^31), and for it SOME shape always is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IDB_FD_HD __host__ __device__ __forceinline__
#else
#define IDB_FD_HD inline
#endif

struct idb_fastdiv {
    uint32_t mul, add, sh;
};

// largest nmax for which q = mulhi(n, ceil(2^32 / d)) is floor(n / d) for every n in [0, nmax]; 2 <= d <= 2^16, d not a power of two
inline uint64_t idb_fastdiv_mulhi_max(uint32_t d) {
    const uint64_t r = ((1ull << 32) + d - 1) / d;
    const uint64_t e = r * d - (1ull << 32);                 // 0 < e < d
    const uint64_t t = ((1ull << 32) + e - 1) / e;           // smallest n with n e >= 2^32
    // the first failing numerator: the smallest n >= t with n % d == d - 1
    const uint64_t first_bad = t + (d - 1 - t % d + d) % d;
    return first_bad - 1;
}

// is ONE multiply-high by ceil(2^32 / d) exact on [0, nmax]?  Powers of two (shifts) and d > 2^16 are not this shape's business.
inline bool idb_fastdiv_mulhi_exact(uint32_t d, uint32_t nmax) {
    if (d < 2 || d > 65536u || (d & (d - 1)) == 0) return false;
    return (uint64_t)nmax <= idb_fastdiv_mulhi_max(d);
}

// {mul, add, sh} for floor(n / d), exact for every n in [0, nmax]; ok = false (and a divisor-1 record) when d == 0, d > 2^31 or nmax >= 2^31
inline idb_fastdiv idb_fastdiv_make(uint32_t d, uint32_t nmax, bool* ok = nullptr) {
    const bool in_range = d != 0 && d <= 0x80000000u && nmax < 0x80000000u;
    if (ok) *ok = in_range;
    if (!in_range) return idb_fastdiv{0u, 0xFFFFFFFFu, 0u};
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;                              // ceil(log2 d)
    if ((d & (d - 1)) == 0) return idb_fastdiv{0u, 0xFFFFFFFFu, l};
    if (idb_fastdiv_mulhi_exact(d, nmax)) return idb_fastdiv{(uint32_t)(((1ull << 32) + d - 1) / d), 0u, 0u};
    const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    return idb_fastdiv{(uint32_t)m, 0xFFFFFFFFu, l};
}

IDB_FD_HD uint32_t idb_fd_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

IDB_FD_HD uint32_t idb_fd_div(uint32_t n, const idb_fastdiv& f) { return (idb_fd_mulhi(n, f.mul) + (n & f.add)) >> f.sh; }

// signed convenience for the kernels' int coordinates (all non-negative there)
IDB_FD_HD int idb_fd_div(int n, const idb_fastdiv& f) { return (int)idb_fd_div((uint32_t)n, f); }
