// cmux.hip -- the CMUX of a ring sample pair under one TGSW selector bit on gfx950 (cmux.hpp has the definition and
// the two bounds).
//
//   cmux_kernel          one workgroup of two wave64 per CMUX; wave q works modulo prime q.  Per input polynomial u: each
//                        lane loads its coefficients of d1[u] - d0[u] (+ the decomposition's offset) once, then for each
//                        of the l digits one forward NTT of the signed digit polynomial and a 64-bit multiply-accumulate
//                        against the two output polynomials of row (u, p)'s image.  After the (k+1) l rows one Montgomery
//                        reduction and inverse NTT per output polynomial; the residues go to LDS in natural order, wave q
//                        then owns output polynomial q: it reads four consecutive coefficients of both primes, applies the
//                        signed CRT, adds d0 and writes 16 bytes per lane and store.
//   cmux_kernel<., true> the rotation step ROT(G, rot, d0) = CMUX(G, X^(-rot) d0, d0) of the packed lookup: the same kernel with
//                        another operand load -- coefficient j of X^(-rot) d0 is d0[j + rot], negated past the wrap -- and
//                        nothing else; d1 and n_d1 are not read.  Lanes read words of d0 other lanes' stores would hit:
//                        launch_cmux refuses an output that overlaps d0.
//   inner_kernel        the product alone, G (.) c, of the encrypted inner products (include/tfhe_hip.h "encrypted inner
//                        products"): the same body with the operand c itself -- no d1 - d0, no + d0 -- and a fused sample
//                        extraction.  After the CRT the torus words go back into LDS over prime 0's residues (every lane
//                        overwrites the 16 bytes it alone has just read), one more barrier, and the two waves write the
//                        rows Extract_(e w), e < S = N / w, of their ring sample in ring_extract_kernel's layout
//                        (unpack.hip): a lane owns 16-byte groups of a row, reads the mask polynomial descending from
//                        A[e w - 4g] in LDS and stores 16 bytes; the last group is (B[e w], 0, 0, 0).  Only rows below M
//                        are written.  The raw test form stores the full product as well (out != null) or alone.
//                        The epilogue starts after the accumulators have died: it adds no register to the body's peak.
// No atomics, no global scratch beyond the row buffer; a CMUX reads nothing another CMUX of the launch writes.
//
// kernels.hip is not touched by this file; the few lines it keeps private (the per-prime context) are restated once, in
// ring_wave.hpp (through cmux.hpp), with inner_kernel's tail, which ring_public.hip shares.
#include "cmux.hpp"

namespace tfhe_hip {

namespace {

// the most rows any accepted gadget has: the accumulators below take that many products (cmux.hpp MAC bound)
static_assert(cmux_mac_ok(1024, 18) && cmux_mac_ok(2048, 16), "rows one accumulator takes");

enum { MODE_CMUX = 0, MODE_ROT = 1, MODE_PRODUCT = 2 };

template <int LOGN, bool ROT_KERNEL>
__global__ __launch_bounds__(128) void cmux_kernel(CmuxArgs a) {
    constexpr int MODE = ROT_KERNEL ? MODE_ROT : MODE_CMUX;
    const RingRows t{};
#include "cmux_body.inc"
}

template <int LOGN>
__global__ __launch_bounds__(128) void inner_kernel(InnerArgs x) {
    constexpr int MODE = MODE_PRODUCT;
    const CmuxArgs &a = x.c;
    const RingRows &t = x.rows;
#include "cmux_body.inc"
}

}  // namespace

bool launch_inner(hipStream_t s, const InnerArgs &x) {
    const CmuxArgs &a = x.c;
    const RingRows &t = x.rows;
    // the gadget as launch_cmux; the operands are the `count` ring samples at d0, 16-byte aligned like every destination
    if (cmux_gadget_error(a.N, 1, a.l, a.Bgbit) || a.bit < 0 || a.bit >= SELECT_MAX_BITS || a.count < 1 || a.stride < 2 * (int64_t)a.N ||
        (a.stride & 3) || !a.d0 || !a.img || !a.tw || a.rot || a.n_d1 || (!a.out && !t.u_buf) || (reinterpret_cast<uintptr_t>(a.out) & 15u))
        return false;
    if (t.u_buf && (ring_rows_error(a.N, a.count, t.M, t.width, t.u_stride) || (reinterpret_cast<uintptr_t>(t.u_buf) & 15u))) return false;
    if (a.N == 2048) hipLaunchKernelGGL((inner_kernel<11>), dim3(a.count), dim3(128), 0, s, x);
    else hipLaunchKernelGGL((inner_kernel<10>), dim3(a.count), dim3(128), 0, s, x);
    return true;
}

bool launch_cmux(hipStream_t s, const CmuxArgs &a) {
    // the kernel is instantiated for k = 1; everything else it was bounded for is checked here once more
    if (cmux_gadget_error(a.N, 1, a.l, a.Bgbit) || a.bit < 0 || a.bit >= SELECT_MAX_BITS || a.count < 1 || a.n_d1 < 0 ||
        a.n_d1 > a.count || a.stride < 2 * (int64_t)a.N || (a.stride & 3) || !a.d0 || (a.n_d1 && !a.d1) || !a.img || !a.tw || !a.out ||
        a.rot < 0 || a.rot >= a.N)
        return false;
    if (a.rot) {
        // a rotation reads d0 across lanes: the words [d0, d0 + (count - 1) stride + 2N) and [out, out + count 2N) stay apart
        const uintptr_t d0b = reinterpret_cast<uintptr_t>(a.d0), outb = reinterpret_cast<uintptr_t>(a.out);
        const uintptr_t d0e = d0b + ((uintptr_t)(a.count - 1) * (uintptr_t)a.stride + 2 * (uintptr_t)a.N) * 4;
        const uintptr_t oute = outb + (uintptr_t)a.count * 2 * (uintptr_t)a.N * 4;
        if (d0b < oute && outb < d0e) return false;
        if (a.N == 2048) hipLaunchKernelGGL((cmux_kernel<11, true>), dim3(a.count), dim3(128), 0, s, a);
        else hipLaunchKernelGGL((cmux_kernel<10, true>), dim3(a.count), dim3(128), 0, s, a);
        return true;
    }
    if (a.N == 2048) hipLaunchKernelGGL((cmux_kernel<11, false>), dim3(a.count), dim3(128), 0, s, a);
    else hipLaunchKernelGGL((cmux_kernel<10, false>), dim3(a.count), dim3(128), 0, s, a);
    return true;
}

}  // namespace tfhe_hip
