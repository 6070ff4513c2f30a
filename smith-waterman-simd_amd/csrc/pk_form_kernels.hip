// pk_form_kernels.hip -- libswmi_pk_form.so (include/swmi_pk_form.h): which cell body the packed scorer runs for a parameter set
// (the rule of pk_form.h, which swmi_api.cpp launches by), and the exhaustive self-test of the flag form's premise.
#include "../../include/swmi_pk_form.h"
#include "pk_form.h"

#include <hip/hip_runtime.h>

namespace {

// sw_kernels.hip keeps the same two constants for the self-test of the non-negative premise (pk_max3_selftest_kernel)
constexpr uint32_t kPkLimit = 0x7C00u;      // first f16 bit pattern that is not a finite number (+Inf)
constexpr uint32_t kBPerThread = 1024;
constexpr uint32_t kNegLow = 0x00FFu;       // the smallest magnitude the flag form produces: 0 + the addend 0x80FF

// The flag form (sw_kernels.hip, "FLAG FORM") hands v_pk_maximum3_f16 a diagonal term 0x80FF + H, H in [0, 0x7C00 - 0xFF): a
// finite NEGATIVE half-precision number, which must lose against the two non-negative operands whatever they are (zero and
// denormal patterns included) and whichever half of the register it sits in.  For EVERY pair (a, b) of 16-bit integers in
// [0, 0x7C00) and pseudo-random magnitudes v, v2 in [0x00FF, 0x7C00) -- drawn as pk_max3_selftest_kernel draws its third value
// -- the result must be the integer max of the non-negative halves: the negative operand in both halves, in the low half only
// and in the high half only (beside a random non-negative r), and in each of the three operand positions (the sweep uses the
// third).  Thread = one a, kBPerThread consecutive b.
__global__ void __launch_bounds__(256)
pk_max3_negative_selftest_kernel(unsigned long long *__restrict__ counts /* [0] checked, [1] mismatches */)
{
    // the integers below 1024 are f16 denormals as bit patterns: keep them, as every kernel that uses the instruction does
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 6, 2), 3");
    const uint32_t a = blockIdx.x * 256 + threadIdx.x;
    const uint32_t b0 = blockIdx.y * kBPerThread;
    if (a >= kPkLimit) return;
    auto pk_max3 = [](uint32_t p, uint32_t q, uint32_t r) {
        uint32_t o;
        asm volatile("v_pk_maximum3_f16 %0, %1, %2, %3\n\ts_nop 1" : "=v"(o) : "v"(p), "v"(q), "v"(r));
        return o;
    };
    uint32_t bad = 0, done = 0;
    for (uint32_t b = b0; b < b0 + kBPerThread && b < kPkLimit; ++b) {
        uint32_t h = (a * 0x9E3779B1u) ^ (b * 0x85EBCA77u);
        h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
        const uint32_t v = kNegLow + h % (kPkLimit - kNegLow), v2 = kNegLow + (h >> 7) % (kPkLimit - kNegLow), r = (h >> 3) % kPkLimit;
        const uint32_t m = a > b ? a : b, mr = m > r ? m : r;
        const uint32_t p = a | (b << 16), q = b | (a << 16);                     // max per half: m, m
        const uint32_t z[3] = {(0x8000u | v) | ((0x8000u | v2) << 16),            // negative in both halves
                               (0x8000u | v) | (r << 16),                         // ... in the low half, r beside it
                               r | ((0x8000u | v2) << 16)};                       // ... in the high half
        const uint32_t want[3] = {m | (m << 16), m | (mr << 16), mr | (m << 16)};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bad += pk_max3(p, q, z[k]) != want[k];       // the sweep's position: max3(left, up, diagonal term)
            bad += pk_max3(p, z[k], q) != want[k];
            bad += pk_max3(z[k], p, q) != want[k];
        }
        done += 9;
    }
    atomicAdd(&counts[0], (unsigned long long)done);
    if (bad) atomicAdd(&counts[1], (unsigned long long)bad);
}

// The product form (sw_kernels.hip, "PRODUCT FORM") takes its diagonal term from v_pk_mad_i16: per half
// a[r] * b[c] + d modulo 2^16, halves independent.  For ALL 16 (r, c), EVERY d in [0, kPkProductBound] and both halves (the other
// half holds another (r, c) and the mirrored d, so that every combination passes through each half) the instruction must give
// the integer formula, and the max3 that follows it in the sweep -- against two pseudo-random non-negative operands -- must
// give max(p, q, d + 255) where r = c and max(p, q) where not.  Thread = one d.
struct ProductMuls {
    uint32_t a[4], b[4];
};
__global__ void __launch_bounds__(256)
pk_product_mad_selftest_kernel(ProductMuls mul, unsigned long long *__restrict__ counts /* [0] checked, [1] mismatches */)
{
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 6, 2), 3");
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d > (uint32_t)swmi::kPkProductBound) return;
    const uint32_t d2 = (uint32_t)swmi::kPkProductBound - d;
    auto imax = [](uint32_t p, uint32_t q) { return p > q ? p : q; };
    uint32_t bad = 0, done = 0;
    for (uint32_t rc = 0; rc < 16; ++rc) {
        const uint32_t rc2 = (rc + 7) % 16, r = rc / 4, c = rc % 4, r2 = rc2 / 4, c2 = rc2 % 4;
        const uint32_t rowmul = mul.a[r] | (mul.a[r2] << 16), colmul = mul.b[c] | (mul.b[c2] << 16), hd = d | (d2 << 16);
        uint32_t t, x;
        asm volatile("v_pk_mad_i16 %0, %1, %2, %3\n\ts_nop 1" : "=v"(t) : "v"(rowmul), "v"(colmul), "v"(hd));
        const uint32_t want_lo = (mul.a[r] * mul.b[c] + d) & 0xFFFFu, want_hi = (mul.a[r2] * mul.b[c2] + d2) & 0xFFFFu;
        bad += t != (want_lo | (want_hi << 16));
        uint32_t hsh = (d * 0x9E3779B1u) ^ (rc * 0x85EBCA77u);
        hsh ^= hsh >> 15; hsh *= 0x2C1B3C6Du; hsh ^= hsh >> 12;
        const uint32_t p_lo = hsh % kPkLimit, p_hi = (hsh >> 5) % kPkLimit, q_lo = (hsh >> 9) % kPkLimit, q_hi = (hsh >> 13) % kPkLimit;
        asm volatile("v_pk_maximum3_f16 %0, %1, %2, %3\n\ts_nop 1" : "=v"(x) : "v"(p_lo | (p_hi << 16)), "v"(q_lo | (q_hi << 16)), "v"(t));
        const uint32_t x_lo = r == c ? imax(imax(p_lo, q_lo), d + 255u) : imax(p_lo, q_lo);
        const uint32_t x_hi = r2 == c2 ? imax(imax(p_hi, q_hi), d2 + 255u) : imax(p_hi, q_hi);
        bad += x != (x_lo | (x_hi << 16));
        done += 2;
    }
    atomicAdd(&counts[0], (unsigned long long)done);
    if (bad) atomicAdd(&counts[1], (unsigned long long)bad);
}

template <typename Launch>
int run_counting_selftest(unsigned long long *checked, unsigned long long *mismatches, Launch launch)
{
    if (!checked || !mismatches) return SWMI_ERR_INVALID_ARGUMENT;
    unsigned long long *d = nullptr, h[2] = {0, 0};
    if (hipMalloc(reinterpret_cast<void **>(&d), sizeof h) != hipSuccess) return SWMI_ERR_HIP;
    hipError_t e = hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch(d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);      // (waits for the kernel)
    (void)hipFree(d);
    if (e != hipSuccess) return SWMI_ERR_HIP;
    *checked = h[0];
    *mismatches = h[1];
    return SWMI_OK;
}

}  // namespace

extern "C" {

int swmi_pk_cell_form(const int8_t score_matrix[16], int gap_penalty, int scale[2])
{
    if (scale) scale[0] = scale[1] = 0;
    if (!score_matrix) return SWMI_ERR_INVALID_ARGUMENT;
    if (gap_penalty < 0 || gap_penalty > 127) return SWMI_ERR_DOMAIN;
    const swmi::PkCellForm f = swmi::pk_cell_form(score_matrix, gap_penalty);
    if (!f.flag_unit) return f.variant;
    if (scale) {
        scale[0] = f.flag_unit;
        scale[1] = f.flag_gap;
    }
    return SWMI_PK_FORM_FLAG;
}

int swmi_pk_selftest_max3_negative(unsigned long long *checked, unsigned long long *mismatches)
{
    return run_counting_selftest(checked, mismatches, [](unsigned long long *d) {
        const dim3 grid((kPkLimit + 255) / 256, (kPkLimit + kBPerThread - 1) / kBPerThread);
        hipLaunchKernelGGL(pk_max3_negative_selftest_kernel, grid, dim3(256), 0, 0, d);
    });
}

int swmi_pk_product_form(const int8_t score_matrix[16], int gap_penalty, int consts[9])
{
    if (consts)
        for (int k = 0; k < 9; ++k) consts[k] = 0;
    if (!score_matrix) return SWMI_ERR_INVALID_ARGUMENT;
    if (gap_penalty < 0 || gap_penalty > 127) return SWMI_ERR_DOMAIN;
    if (!swmi::pk_cell_form(score_matrix, gap_penalty).product) return 0;
    if (consts) {
        for (int k = 0; k < 4; ++k) {
            consts[k] = swmi::kPkProductRowMul[k];
            consts[4 + k] = swmi::kPkProductColMul[k];
        }
        consts[8] = swmi::kPkProductBound;
    }
    return 1;
}

int swmi_pk_selftest_product_mad(unsigned long long *checked, unsigned long long *mismatches)
{
    return run_counting_selftest(checked, mismatches, [](unsigned long long *d) {
        ProductMuls mul;
        for (int k = 0; k < 4; ++k) {
            mul.a[k] = swmi::kPkProductRowMul[k];
            mul.b[k] = swmi::kPkProductColMul[k];
        }
        hipLaunchKernelGGL(pk_product_mad_selftest_kernel, dim3((swmi::kPkProductBound + 256) / 256), dim3(256), 0, 0, mul, d);
    });
}

}  // extern "C"
