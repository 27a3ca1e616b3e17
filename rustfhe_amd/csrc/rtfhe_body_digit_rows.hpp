// rtfhe_body_digit_rows.hpp -- the digit-row loop of the external product: text, no include guard, included where the loop runs (the idiom of
// rtfhe_body_pair.hpp; a __device__ helper in its place changed the code of every kernel built on cmux_step).
//
// This is the SINGLE statement of the loop every bit-exactness guarantee rests on (hadamard + fold-add from zero,
// utils/src/spqlios.rs:204-222, hom_nand/src/trgsw.rs:290-299): for each digit jj of the polynomial whose pre-masked words are in u, the
// digits, fft_forward_a, the digit's two key rows, fft_forward_b, then the unfused rr - ii, ir + ri fold-add into s0* and s1*.  Included by
// cmux_step (rtfhe_kernels.hpp), mac_forward (rtfhe_kernels_trgsw_mac.hpp) and auto_step (rtfhe_kernels_trlwe_auto.hpp); mb_step
// (rtfhe_kernels_pbs_mb.hpp) mirrors it with the key combination in the fold.
//
// The includer has declared: u[2 R] (the polynomial's words after (x + MA) ^ MX), R, L, BGBIT, LOGN, DUAL, twf, xbuf, lane and the four
// running spectra s0re, s0im, s1re, s1im [R].  It defines ONE macro, RTFHE_DIGIT_ROW(jj): the const cplx* (lane already added) of digit jj's
// row pair, [2][R][64]; the body #undefs it at its end.
#pragma unroll 1
        for (int jj = 0; jj < L; jj++) {
            const cplx* bkj = RTFHE_DIGIT_ROW(jj);
            double re[R], im[R];
#pragma unroll
            for (int m = 0; m < R; m++) {
                re[m] = (double)decomp_digit(u[m], BGBIT, jj);
                im[m] = (double)decomp_digit(u[R + m], BGBIT, jj);
            }
            fft_forward_a<LOGN, DUAL>(re, im, twf, xbuf, lane);
            // the two key rows of this digit are requested here, not earlier: their 64 VGPRs would otherwise be
            // live through the whole transform; the last exchange + in-register pass cover the L2 latency
            __builtin_amdgcn_sched_barrier(0);
            cplx b0[R], b1[R];
#pragma unroll
            for (int m = 0; m < R; m++) { b0[m] = bkj[m * 64]; b1[m] = bkj[(R + m) * 64]; }
            __builtin_amdgcn_sched_barrier(0);
            fft_forward_b<LOGN, DUAL>(re, im, twf, xbuf, lane);
#pragma unroll
            for (int m = 0; m < R; m++) {
                {
                    const double ii = b0[m].y * im[m], rr = b0[m].x * re[m], ri = b0[m].x * im[m], ir = b0[m].y * re[m];
                    s0re[m] = s0re[m] + (rr - ii);
                    s0im[m] = s0im[m] + (ir + ri);
                }
                {
                    const double ii = b1[m].y * im[m], rr = b1[m].x * re[m], ri = b1[m].x * im[m], ir = b1[m].y * re[m];
                    s1re[m] = s1re[m] + (rr - ii);
                    s1im[m] = s1im[m] + (ir + ri);
                }
            }
        }
#undef RTFHE_DIGIT_ROW
