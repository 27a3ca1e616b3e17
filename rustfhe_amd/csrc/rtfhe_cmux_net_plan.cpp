// rtfhe_cmux_net_plan.cpp -- host only: the checks and the levelisation of a CMUX netlist (rtfhe_cmux_net_plan.h), before
// rtfhe_cmux_circuit_create (rtfhe_cmux_net.hip) allocates or launches anything.
#include "rtfhe_cmux_net_plan.h"

#include <vector>

#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

extern "C" int rtfhe_cmux_net_plan(const rtfhe_cmux_net_world* w, const int32_t* var, const int32_t* hi, const int32_t* lo, const int32_t* rot,
                                   int32_t n_nodes, int32_t n_vars, const int32_t* out_ref, const int32_t* out_coef, int32_t n_out,
                                   int32_t* order, int32_t* level_off, int32_t* n_levels, int32_t* leaf_span, size_t* node_bytes, char* err,
                                   size_t err_len) {
    begin(err, err_len);
    if (!w || !var || !hi || !lo || !out_ref || !order || !level_off || !n_levels || !leaf_span || !node_bytes)
        return refuse(err, err_len, "rtfhe_cmux_circuit_create: null argument");
    if (n_nodes < 1 || n_vars < 1 || n_out < 1 || w->count < 1)
        return refuse(err, err_len, "rtfhe_cmux_circuit_create: n_nodes, n_vars, n_out and count must be at least 1");
    const long long N = w->N, n_lut = w->n_lut;
    long long leaf_min = -1, leaf_max = -1;
    std::vector<int32_t> level((size_t)n_nodes, 0);
    int32_t deepest = 0;
    for (int32_t i = 0; i < n_nodes; i++) {
        const std::string at = "node " + num(i) + ": ";
        if (var[i] < 0 || var[i] >= n_vars) return refuse(err, err_len, at + "var = " + num(var[i]) + " is outside [0, " + num(n_vars) + ")");
        int32_t lv = 0;
        const int32_t refs[2] = {hi[i], lo[i]};
        for (int k = 0; k < 2; k++) {
            const long long r = refs[k];
            const char* name = k ? "lo" : "hi";
            if (r >= 0) {
                if (r >= i)
                    return refuse(err, err_len, at + name + " = " + num(r) + " is not an earlier node (the nodes are in topological order: a reference is below " +
                                                    num(i) + ")");
                if (level[(size_t)r] + 1 > lv) lv = level[(size_t)r] + 1;
            } else {
                const long long leaf = -1 - r;
                if (!w->has_row0 && leaf >= n_lut)
                    return refuse(err, err_len, at + name + " = " + num(r) + " is table row " + num(leaf) + ", the table has " + num(n_lut));
                if (leaf_min < 0 || leaf < leaf_min) leaf_min = leaf;
                if (leaf > leaf_max) leaf_max = leaf;
            }
        }
        if (rot && (rot[i] < 0 || rot[i] >= 2 * N)) return refuse(err, err_len, at + "rot = " + num(rot[i]) + " is outside [0, " + num(2 * N) + ")");
        level[(size_t)i] = lv;
        if (lv > deepest) deepest = lv;
    }
    for (int32_t o = 0; o < n_out; o++) {
        const std::string at = "output " + num(o) + ": ";
        if (out_ref[o] < 0) return refuse(err, err_len, at + "out_ref = " + num(out_ref[o]) + " names a table row; an output is a node");
        if (out_ref[o] >= n_nodes) return refuse(err, err_len, at + "out_ref = " + num(out_ref[o]) + " is outside [0, " + num(n_nodes) + ")");
        if (out_coef && (out_coef[o] < 0 || out_coef[o] >= N))
            return refuse(err, err_len, at + "out_coef = " + num(out_coef[o]) + " is outside [0, " + num(N) + ")");
    }
    if (!w->has_sel_idx && (w->count > (size_t)w->n_sel / (size_t)n_vars))
        return refuse(err, err_len, "sel_idx NULL: replica " + num((long long)w->count - 1) + " needs selectors up to " + num((long long)w->count - 1) + " * " +
                                        num(n_vars) + " + " + num(n_vars - 1) + ", the set has " + num(w->n_sel));
    // count * n_nodes * 2N words of 4 bytes, and count * max(n_nodes, n_out) waves per launch as a 32-bit number
    const size_t per = (size_t)n_nodes * 2 * (size_t)N * 4, most = n_nodes > n_out ? (size_t)n_nodes : (size_t)n_out;
    if (w->count > (size_t)-1 / per) return refuse(err, err_len, "the node buffer count * n_nodes * 8N bytes does not fit size_t");
    if (!count_fits(w->count, most)) return refuse(err, err_len, "count * max(n_nodes, n_out) too large");
    *node_bytes = w->count * per;
    // counting sort by level: index order within a level
    const int32_t levels = deepest + 1;
    for (int32_t k = 0; k <= levels; k++) level_off[k] = 0;
    for (int32_t i = 0; i < n_nodes; i++) level_off[level[(size_t)i] + 1]++;
    for (int32_t k = 0; k < levels; k++) level_off[k + 1] += level_off[k];
    std::vector<int32_t> next(level_off, level_off + levels);
    for (int32_t i = 0; i < n_nodes; i++) order[next[(size_t)level[(size_t)i]]++] = i;
    *n_levels = levels;
    leaf_span[0] = (int32_t)leaf_min;
    leaf_span[1] = (int32_t)leaf_max;
    return 0;
}
