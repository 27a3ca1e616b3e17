/* Walks the host-only part of rtfhe_cmux_circuit_create (rustfhe_amd/csrc/rtfhe_cmux_net_plan.cpp: every check of a CMUX netlist's
 * description, and its levelisation) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: this code runs before any HIP
 * call.  The output arrays are allocated at exactly the sizes the header promises, so that a write past them is caught. */
#include <limits.h>
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_cmux_net_plan.h"

typedef struct { int32_t *order, *level_off, n_levels, leaf_span[2]; size_t node_bytes; char err[200]; } plan_out;

static int plan(const rtfhe_cmux_net_world *w, const int32_t *var, const int32_t *hi, const int32_t *lo, const int32_t *rot, int32_t n_nodes, int32_t n_vars,
                const int32_t *out_ref, const int32_t *out_coef, int32_t n_out, plan_out *p) {
    const size_t nn = n_nodes > 0 ? (size_t)n_nodes : 1;
    p->order = malloc(sizeof(int32_t) * nn);
    p->level_off = malloc(sizeof(int32_t) * (nn + 1));
    CHECK(p->order && p->level_off);
    memset(p->err, 'x', sizeof p->err);
    return rtfhe_cmux_net_plan(w, var, hi, lo, rot, n_nodes, n_vars, out_ref, out_coef, n_out, p->order, p->level_off, &p->n_levels, p->leaf_span,
                               &p->node_bytes, p->err, sizeof p->err);
}
static void done(plan_out *p) { free(p->order); free(p->level_off); }

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
/* (a netlist has no caller buffers: the item rule and the node buffer's size in bytes) */
static size_t large_node_bytes;
static int large_plan(size_t count, const void *in, const void *out) {
    const rtfhe_cmux_net_world lw = {1024, 2, 1, 1, 1, count};
    const int32_t v[1] = {0}, h[1] = {-1}, l[1] = {-2}, o[1] = {0};
    int32_t order[1], level_off[2], n_levels, span[2];
    (void)in; (void)out;
    memset(err, 'x', sizeof err);
    return rtfhe_cmux_net_plan(&lw, v, h, l, NULL, 1, 1, o, NULL, 1, order, level_off, &n_levels, span, &large_node_bytes, err, sizeof err);
}

int main(void) {
    const rtfhe_cmux_net_world w = {1024, 23, 185, 0, 0, 37};
    /* the mixed netlist of the GPU test's shape: 11 nodes on 5 variables, levels of 4, 3, 3 and 1 nodes */
    const int32_t var[11] = {0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0};
    const int32_t hi[11] = {-2, -4, -6, -1, 0, 1, -7, 4, -8, 5, 7};
    const int32_t lo[11] = {-1, -3, -5, -1, 1, -5, 2, 5, 6, 5, 8};
    const int32_t rot[11] = {0, 1, 1024, 2047, 0, 3, 0, 0, 17, 5, 0};
    const int32_t out_ref[3] = {10, 4, 9}, out_coef[3] = {0, 1, 1023};
    plan_out p;
    CHECK(plan(&w, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p) == 0 && p.err[0] == 0);
    CHECK(p.n_levels == 4 && p.level_off[0] == 0 && p.level_off[1] == 4 && p.level_off[2] == 7 && p.level_off[3] == 10 && p.level_off[4] == 11);
    {
        const int32_t want[11] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
        CHECK(!memcmp(p.order, want, sizeof want));
    }
    CHECK(p.leaf_span[0] == 0 && p.leaf_span[1] == 7 && p.node_bytes == (size_t)37 * 11 * 2 * 1024 * 4);
    done(&p);
    CHECK(plan(&w, var, hi, lo, NULL, 11, 5, out_ref, NULL, 3, &p) == 0);          /* rot NULL, TRLWE form */
    done(&p);
    {   /* a chain: as many levels as nodes, level_off is written up to [n_nodes] */
        enum { D = 64 };
        int32_t v[D], h[D], o = D - 1;
        for (int i = 0; i < D; i++) { v[i] = i % 5; h[i] = i - 1; }
        CHECK(plan(&w, v, h, h, NULL, D, 5, &o, NULL, 1, &p) == 0 && p.n_levels == D && p.level_off[D] == D && p.order[D - 1] == D - 1);
        CHECK(p.leaf_span[0] == 0 && p.leaf_span[1] == 0);
        done(&p);
    }
    {   /* a late node of a low level: sorted by level, index order within it */
        const int32_t v[4] = {0, 1, 2, 0}, h[4] = {-1, 0, 1, -3}, l[4] = {-2, -2, 0, -1}, o = 2, want[4] = {0, 3, 1, 2};
        CHECK(plan(&w, v, h, l, NULL, 4, 3, &o, NULL, 1, &p) == 0 && p.n_levels == 3 && !memcmp(p.order, want, sizeof want));
        CHECK(p.level_off[1] == 2 && p.level_off[2] == 3 && p.level_off[3] == 4 && p.leaf_span[1] == 2);
        done(&p);
    }
    /* refusals: every one names its node or output and writes nothing past err */
#define REFUSED(call, text) do { CHECK((call) == RTFHE_ERR_INVALID); CHECK(strstr(p.err, text)); CHECK(strlen(p.err) < sizeof p.err); done(&p); } while (0)
    {
        int32_t b[11];
        memcpy(b, var, sizeof b); b[7] = 5;
        REFUSED(plan(&w, b, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "node 7: var = 5");
        b[7] = -1;
        REFUSED(plan(&w, b, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "node 7: var = -1");
        memcpy(b, hi, sizeof b); b[4] = 4;
        REFUSED(plan(&w, var, b, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "node 4: hi = 4");          /* itself */
        b[4] = 9;
        REFUSED(plan(&w, var, b, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "node 4: hi = 9");          /* a forward reference */
        b[4] = INT_MAX;
        REFUSED(plan(&w, var, b, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "node 4: hi");
        memcpy(b, lo, sizeof b); b[10] = -24;
        REFUSED(plan(&w, var, hi, b, rot, 11, 5, out_ref, out_coef, 3, &p), "node 10: lo = -24 is table row 23");
        b[10] = INT_MIN;
        REFUSED(plan(&w, var, hi, b, rot, 11, 5, out_ref, out_coef, 3, &p), "node 10: lo");
        memcpy(b, rot, sizeof b); b[3] = 2048;
        REFUSED(plan(&w, var, hi, lo, b, 11, 5, out_ref, out_coef, 3, &p), "node 3: rot = 2048");
        b[3] = -1;
        REFUSED(plan(&w, var, hi, lo, b, 11, 5, out_ref, out_coef, 3, &p), "node 3: rot = -1");
    }
    {
        int32_t o[3] = {10, -1, 9}, c[3] = {0, 1, 1024};
        REFUSED(plan(&w, var, hi, lo, rot, 11, 5, o, out_coef, 3, &p), "output 1: out_ref = -1 names a table row");
        o[1] = 11;
        REFUSED(plan(&w, var, hi, lo, rot, 11, 5, o, out_coef, 3, &p), "output 1: out_ref = 11");
        REFUSED(plan(&w, var, hi, lo, rot, 11, 5, out_ref, c, 3, &p), "output 2: out_coef = 1024");
        c[2] = -1;
        REFUSED(plan(&w, var, hi, lo, rot, 11, 5, out_ref, c, 3, &p), "output 2: out_coef = -1");
    }
    {
        rtfhe_cmux_net_world v = w;
        v.n_sel = 5 * 37 - 1;                                                    /* one selector short */
        REFUSED(plan(&v, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "sel_idx NULL: replica 36");
        v.has_sel_idx = 1;
        CHECK(plan(&v, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p) == 0);
        done(&p);
        v = w; v.n_lut = 7;                                                      /* row 7 is past it ... */
        REFUSED(plan(&v, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "is table row 7, the table has 7");
        v.has_row0 = 1;                                                          /* ... unless row0 lives on the device */
        {
            int32_t b[11];
            memcpy(b, lo, sizeof b); b[10] = INT_MIN;
            CHECK(plan(&v, var, hi, b, rot, 11, 5, out_ref, out_coef, 3, &p) == 0 && p.leaf_span[1] == INT_MAX);
            done(&p);
        }
        v = w; v.has_sel_idx = 1; v.count = (size_t)-1 / 8;                      /* the node buffer's bytes pass size_t */
        REFUSED(plan(&v, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "does not fit size_t");
        v.count = (size_t)0x7fffffff / 11 + 1;
        REFUSED(plan(&v, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "too large");
        v.count = 0;
        REFUSED(plan(&v, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "at least 1");
    }
    REFUSED(plan(&w, var, hi, lo, rot, 0, 5, out_ref, out_coef, 3, &p), "at least 1");
    REFUSED(plan(&w, var, hi, lo, rot, 11, 0, out_ref, out_coef, 3, &p), "at least 1");
    REFUSED(plan(&w, var, hi, lo, rot, 11, 5, out_ref, out_coef, 0, &p), "at least 1");
    REFUSED(plan(&w, NULL, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "null argument");
    REFUSED(plan(NULL, var, hi, lo, rot, 11, 5, out_ref, out_coef, 3, &p), "null argument");
    {   /* a message longer than the caller's buffer is cut, not overrun */
        int32_t b[11];
        char small[8];
        int32_t order[11], off[12], nl, span[2];
        size_t nb;
        memcpy(b, var, sizeof b); b[7] = 5;
        CHECK(rtfhe_cmux_net_plan(&w, b, hi, lo, rot, 11, 5, out_ref, out_coef, 3, order, off, &nl, span, &nb, small, sizeof small) == RTFHE_ERR_INVALID);
        CHECK(strlen(small) == sizeof small - 1 && !strcmp(small, "node 7:"));
        CHECK(rtfhe_cmux_net_plan(&w, b, hi, lo, rot, 11, 5, out_ref, out_coef, 3, order, off, &nl, span, &nb, NULL, 0) == RTFHE_ERR_INVALID);
    }
    large_limit(large_plan, 0x7fffffff, 0, "count * max(n_nodes, n_out)");
    CHECK(large_plan(((size_t)1 << 21) + 3, NULL, NULL) == 0 && large_node_bytes == (((size_t)1 << 21) + 3) * 8192);
    printf("cmux net sanitizer walk ok\n");
    return 0;
}
