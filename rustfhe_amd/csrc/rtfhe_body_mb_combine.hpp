// rtfhe_body_mb_combine.hpp -- the key combination of the multi-bit step for one component of one digit row: text, no include guard, included
// where it runs (the idiom of rtfhe_body_digit_rows.hpp; as a __device__ __forceinline__ function the six k_pbs_mb* kernels came out with
// the operands of two scalar adds swapped, and the rule is equal device code).
//
// The SINGLE statement for both kernel shapes, mb_step's fold (rtfhe_kernels_pbs_mb.hpp) and k_pbs_mb_wg's product
// (rtfhe_kernels_pbs_mb_wg.hpp):  K = F_{e_1} B_1;  K = K + F_{e_j} B_j for j = 2 .. J, every complex product (rr - ii, ir + ri) and every sum
// rounded on its own, in this order.  No subset is skipped when e_j = 0.
//
// The includer has declared: K[R] (the result), b[R] (subset 1's row of the component, already in registers), row (subset 1's row pair,
// + lane: the further subsets' rows are read from it one at a time), comp, J, r0, r1, r2, roots, q[R], R, MASK and TRGSW.
#pragma unroll
                for (int m = 0; m < R; m++) {
                    const cplx w = roots[(r0 * q[m]) & MASK];
                    const double fx = w.x - 1.0, fy = w.y;
                    const double ii = fy * b[m].y, rr = fx * b[m].x, ri = fx * b[m].y, ir = fy * b[m].x;
                    K[m].x = rr - ii;
                    K[m].y = ir + ri;
                }
#pragma unroll 1
                for (int j = 2; j <= J; j++) {
                    const int e = mb_exponent(j, r0, r1, r2, MASK);
                    const cplx* bj = row + (size_t)(j - 1) * TRGSW + (size_t)comp * R * 64;
#pragma unroll
                    for (int m = 0; m < R; m++) {
                        const cplx v = bj[m * 64];
                        const cplx w = roots[(e * q[m]) & MASK];
                        const double fx = w.x - 1.0, fy = w.y;
                        const double ii = fy * v.y, rr = fx * v.x, ri = fx * v.y, ir = fy * v.x;
                        K[m].x = K[m].x + (rr - ii);
                        K[m].y = K[m].y + (ir + ri);
                    }
                }
