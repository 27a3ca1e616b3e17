/* rtfhe_cmux_net_plan.h -- the host-only part of rtfhe_cmux_circuit_create (include/rtfhe.h): every check of a CMUX netlist's description
 * and its levelisation, with no device call in it (rtfhe_cmux_net_plan.cpp).  Internal: rtfhe_cmux_net.hip calls it before anything is
 * allocated, and tests/c/cmux_net_sanitize_main.c walks it under the host sanitizers.  Plain C so that a C host can include it. */
#ifndef RTFHE_CMUX_NET_PLAN_H
#define RTFHE_CMUX_NET_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* What the netlist is checked against: the ring degree, the table's rows (n_lut; has_row0: row0 lives on the device, so only the kernel can
 * check the row range), the selector set's size (n_sel; has_sel_idx: as for row0) and the batch's replicas. */
typedef struct {
    int32_t N, n_lut, n_sel;
    int32_t has_row0, has_sel_idx;
    size_t count;
} rtfhe_cmux_net_world;

/* Checks var / hi / lo / rot (NULL: all zero) of n_nodes nodes over n_vars variables and the n_out outputs (out_coef NULL: TRLWE form), in
 * the order rtfhe.h lists, and levelises: level(i) = 1 + the largest level of its node children, 0 for a node with only leaf children.
 *   order      [n_nodes]      the nodes sorted by level, index order within a level
 *   level_off  [n_nodes + 1]  level k is order[level_off[k] .. level_off[k + 1]); entries past *n_levels are not written
 *   leaf_span  [2]            the smallest and the largest leaf number -1 - r the netlist names
 *   node_bytes                count * n_nodes * 2N * 4, the node buffer
 * Returns 0, or RTFHE_ERR_INVALID with a message naming the node or output in err (always terminated; err_len >= 1). */
int rtfhe_cmux_net_plan(const rtfhe_cmux_net_world *w, const int32_t *var, const int32_t *hi, const int32_t *lo, const int32_t *rot,
                        int32_t n_nodes, int32_t n_vars, const int32_t *out_ref, const int32_t *out_coef, int32_t n_out,
                        int32_t *order, int32_t *level_off, int32_t *n_levels, int32_t *leaf_span, size_t *node_bytes, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif

#endif
