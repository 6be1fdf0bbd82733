"""idb_fastdiv.h — the launch-constant divisions of the GEMM kernels — checked on the host (no GPU): a stand-alone C++ program includes
the header and compares quotient and remainder with `/` and `%`.

  * every divisor 1 .. 4096 plus the sizes the callers divide by (pixel counts 49 / 144 / 196 / 784 / 3136 / 9216 / 12544, column-tile and
    channel counts 160 k) against the numerators 0, 1, d - 1, d, d + 1, every multiple of d +- 1 up to 2^20, and 2^31 - 1 with its
    neighbours — in the shape idb_fastdiv_make picks for the range the GEMM host code admits (n < 2^31) and, where the one-multiply
    shape is exact on a smaller range, in that shape on that range;
  * the host-side exact-range predicate of the one-multiply shape: for every such divisor the first numerator whose multiply-high
    quotient is wrong is found by a search that does not use the header's formula (the quotient error is monotone along each residue
    class, so a bisection over the multiples of d minus one finds it, and a brute-force scan confirms that no other numerator below it
    fails), and idb_fastdiv_mulhi_exact must say yes for every range below it and no from it on;
  * idb_fastdiv_make refuses a zero divisor and ranges from 2^31 on."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faceposegenerator_amd", "csrc")

PROGRAM = r"""
#include "idb_fastdiv.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static long long failures = 0;
static void fail(const char* what, uint32_t d, uint64_t n, uint64_t got, uint64_t want) {
    if (++failures <= 20) printf("FAIL %s d=%u n=%llu got=%llu want=%llu\n", what, d, (unsigned long long)n, (unsigned long long)got, (unsigned long long)want);
}

static void check_one(const char* what, uint32_t d, const idb_fastdiv& f, uint32_t n) {
    const uint32_t q = idb_fd_div(n, f), r = n - q * d;
    if (q != n / d || r != n % d) fail(what, d, n, q, n / d);
}

// the numerators of the issue, clipped to [0, nmax]
static void check_range(const char* what, uint32_t d, const idb_fastdiv& f, uint32_t nmax) {
    const uint32_t fixed[] = {0u, 1u, d - 1u, d, d + 1u, 0x7FFFFFFFu, 0x7FFFFFFEu, 0x7FFFFFFDu, 0x7FFFFFFFu - d, 0x7FFFFFFFu / d * d, 0x7FFFFFFFu / d * d - 1u};
    for (uint32_t n : fixed)
        if (n <= nmax) check_one(what, d, f, n);
    for (uint64_t m = d; m <= (1u << 20) + (uint64_t)d; m += d)
        for (int o = -1; o <= 1; ++o)
            if (m + o <= nmax) check_one(what, d, f, (uint32_t)(m + o));
    if (nmax >= 2) {
        check_one(what, d, f, nmax);
        check_one(what, d, f, nmax - 1);
    }
}

static bool mulhi_right(uint32_t d, uint32_t r, uint64_t n) { return (uint32_t)((n * r) >> 32) == n / d; }

// first numerator (< 2^32) whose one-multiply quotient is wrong, found without the header's formula; 2^32 if there is none
static uint64_t first_bad_by_search(uint32_t d) {
    const uint32_t r = (uint32_t)(((1ull << 32) + d - 1) / d);
    // residue d - 1: n = k d + d - 1; the error n e / (d 2^32) grows with k, so "wrong" is monotone in k
    uint64_t lo = 0, hi = ((1ull << 32) - d) / d;            // k range with n < 2^32
    if (mulhi_right(d, r, hi * d + d - 1)) return 1ull << 32;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (mulhi_right(d, r, mid * d + d - 1)) lo = mid + 1; else hi = mid;
    }
    return lo * d + d - 1;
}

int main() {
    std::vector<uint32_t> ds;
    for (uint32_t d = 1; d <= 4096; ++d) ds.push_back(d);
    const uint32_t sizes[] = {49, 144, 196, 784, 3136, 9216, 12544};
    for (uint32_t d : sizes) ds.push_back(d);
    for (uint32_t k = 1; k <= 64; ++k) ds.push_back(160 * k);
    long long one_mul = 0, shifts = 0, fallback = 0;
    for (uint32_t d : ds) {
        bool ok = false;
        const idb_fastdiv f = idb_fastdiv_make(d, 0x7FFFFFFFu, &ok);
        if (!ok) fail("make refused", d, 0x7FFFFFFFu, 0, 1);
        check_range("full range", d, f, 0x7FFFFFFFu);
        if (f.mul == 0) ++shifts; else if (f.add == 0) ++one_mul; else ++fallback;
        if (d < 2 || (d & (d - 1)) == 0) {
            if (idb_fastdiv_mulhi_exact(d, 1000u)) fail("predicate accepts a power of two", d, 1000, 1, 0);
            continue;
        }
        // ---- the exact-range predicate of the one-multiply shape
        const uint64_t bad = first_bad_by_search(d);
        const uint32_t r = (uint32_t)(((1ull << 32) + d - 1) / d);
        if (bad < (1ull << 32)) {
            if (mulhi_right(d, r, bad)) fail("search: not a failure", d, bad, 0, 0);
            if (idb_fastdiv_mulhi_max(d) != bad - 1) fail("mulhi_max", d, bad, idb_fastdiv_mulhi_max(d), bad - 1);
            if (!idb_fastdiv_mulhi_exact(d, (uint32_t)(bad - 1))) fail("predicate refuses an exact range", d, bad - 1, 0, 1);
            if (idb_fastdiv_mulhi_exact(d, (uint32_t)bad)) fail("predicate accepts a wrong quotient", d, bad, 1, 0);
            if (bad + 12345 < (1ull << 32) && idb_fastdiv_mulhi_exact(d, (uint32_t)(bad + 12345))) fail("predicate accepts beyond", d, bad + 12345, 1, 0);
        } else if (idb_fastdiv_mulhi_max(d) < 0xFFFFFFFFull) {
            fail("mulhi_max too small", d, 0, idb_fastdiv_mulhi_max(d), 0xFFFFFFFFull);
        }
        // the one-multiply record on the largest range it is exact on
        const uint32_t nmax = (uint32_t)(bad - 1 < 0x7FFFFFFFull ? bad - 1 : 0x7FFFFFFFull);
        const idb_fastdiv g = idb_fastdiv_make(d, nmax, &ok);
        if (!ok || g.add != 0 || g.sh != 0 || g.mul != r) fail("make did not pick the one-multiply shape", d, nmax, g.mul, r);
        check_range("one multiply", d, g, nmax);
    }
    // brute force below the first failure (every numerator, not only residue d - 1), on divisors with early failures and the callers' sizes
    const uint32_t brute[] = {3, 7, 49, 144, 196, 641, 784, 1025, 3136, 4095, 9216, 12544, 160 * 33};
    for (uint32_t d : brute) {
        const uint32_t r = (uint32_t)(((1ull << 32) + d - 1) / d);
        const uint64_t bad = first_bad_by_search(d), end = bad < (1ull << 25) ? bad : (1ull << 25);
        for (uint64_t n = 0; n < end; ++n)
            if (!mulhi_right(d, r, n)) { fail("a failure below the first failure", d, n, 0, 0); break; }
    }
    // refusals
    bool ok = true;
    idb_fastdiv_make(0, 100, &ok);
    if (ok) fail("make accepts d = 0", 0, 0, 1, 0);
    idb_fastdiv_make(7, 0x80000000u, &ok);
    if (ok) fail("make accepts nmax = 2^31", 7, 0x80000000u, 1, 0);
    // large divisors (the fallback shape up to 2^31)
    const uint32_t big[] = {65537u, 1000003u, 0x3FFFFFFFu, 0x40000001u, 0x7FFFFFFFu, 0x80000000u};
    for (uint32_t d : big) {
        const idb_fastdiv f = idb_fastdiv_make(d, 0x7FFFFFFFu, &ok);
        if (!ok) fail("make refused a large divisor", d, 0, 0, 1);
        check_range("large divisor", d, f, 0x7FFFFFFFu);
    }
    printf("divisors %zu: shifts %lld, one multiply %lld, fallback %lld; failures %lld\n", ds.size(), shifts, one_mul, fallback, failures);
    return failures ? 1 : 0;
}
"""


def _compiler():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    default = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    for cand in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++"), shutil.which("c++")):
        if cand and shutil.which(cand):
            return [shutil.which(cand), "-x", "c++"]
    for cand in (os.environ.get("HIPCC"), default, shutil.which("hipcc")):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return [cand, "-x", "c++"]          # as plain C++: the header needs nothing of HIP on the host
    return None


def test_fastdiv_against_division(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler found")
    src = tmp_path / "fastdiv_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "fastdiv_check"
    c = subprocess.run(cxx + ["-std=c++17", "-O2", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"shifts (\d+), one multiply (\d+), fallback (\d+); failures 0", r.stdout)
    assert m, r.stdout[-500:]
    # over n < 2^31 all three shapes must occur, or the test checks less than it says
    assert all(int(x) > 0 for x in m.groups()), m.groups()
