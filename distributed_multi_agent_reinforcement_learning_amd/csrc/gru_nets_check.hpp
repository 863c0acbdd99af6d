// Host only: the argument checks of the multi-net GRU entry points (include/mappo_ops.h gru_seq_*_multi, gru_seq_split_*_multi,
// gru_cell_fwd_multi, gru_cell_split_fwd_multi).  The fp32 route (csrc/mappo_ops.hip) and the split-bf16 route (csrc/mappo_split.hip,
// csrc/mappo_ops.hip) take the same records and refuse the same calls: one table each, held by tests/test_gru_nets_check_cpu.py.
// A check returns false where the entry point returns MO_ERR_BAD_ARG; it touches no device and dereferences none of the pointers.
#pragma once
#include <stdint.h>

#include "mappo_ops.h"

constexpr int GRU_NETS_H = 128;   // the one hidden size of both kernel families (GRU_H, SBR_H)

template <class... P> inline bool gru_all_set(P... p) { return (... && (p != nullptr)); }
template <class... P> inline bool gru_aligned16(P... p) { return ((... | (uintptr_t)p) & 15) == 0; }   // NULL counts as aligned

inline bool gru_seq_scalars_ok(int32_t n_nets, const void *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents) {
    return n_nets >= 1 && n_nets <= MO_GRU_MAX_NETS && nets && T >= 1 && B >= 1 && H == GRU_NETS_H && gi_agents >= 0 && !(gi_agents && B % gi_agents);
}

// a record's own number of sequences: 0 (the launch's B) .. B, whole teams in the encoder's row order
inline bool gru_net_rows_ok(int32_t mB, int32_t B, int32_t gi_agents) { return mB >= 0 && mB <= B && !(gi_agents && mB % gi_agents); }

inline bool gru_seq_nets_ok(int32_t n_nets, const mo_gru_seq_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents) {
    if (!gru_seq_scalars_ok(n_nets, nets, T, B, H, gi_agents)) return false;
    for (int k = 0; k < n_nets; k++) {
        const mo_gru_seq_net &m = nets[k];
        if (!gru_all_set(m.gi, m.w_hh, m.b_hh, m.h0, m.out) || !gru_aligned16(m.gi, m.w_hh, m.b_hh, m.h0, m.out, m.save)) return false;
        if (!gru_net_rows_ok(m.B, B, gi_agents)) return false;
    }
    return true;
}

inline bool gru_seq_bwd_nets_ok(int32_t n_nets, const mo_gru_seq_bwd_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents) {
    if (!gru_seq_scalars_ok(n_nets, nets, T, B, H, gi_agents)) return false;
    for (int k = 0; k < n_nets; k++) {
        const mo_gru_seq_bwd_net &m = nets[k];
        if (!gru_all_set(m.dout, m.save, m.out, m.h0, m.w_hh, m.dgi, m.dh0)) return false;
        if ((m.dgh == nullptr) == (m.dnr == nullptr)) return false;        // exactly one of the two forms
        if ((m.db_ih || m.db_hh) && !gru_all_set(m.db_ih, m.db_hh, m.workspace)) return false;
        if (!gru_aligned16(m.dout, m.save, m.out, m.h0, m.dgi, m.dgh, m.dnr, m.dh0, m.workspace)) return false;
        if (!gru_net_rows_ok(m.B, B, gi_agents)) return false;
    }
    return true;
}

// split_cell: the split-bf16 cell stores h_out in 16-byte pieces and two of its workgroups share a row tile, so not in place
inline bool gru_cell_nets_ok(int32_t n_nets, const mo_gru_cell_net *nets, int32_t B, int32_t H, bool split_cell) {
    if (n_nets < 1 || n_nets > MO_GRU_CELL_MAX_NETS || !nets || B < 1 || H != GRU_NETS_H) return false;
    for (int k = 0; k < n_nets; k++) {
        const mo_gru_cell_net &m = nets[k];
        if (!gru_all_set(m.x, m.h_prev, m.w_ih, m.w_hh, m.b_ih, m.b_hh, m.h_out) || !gru_aligned16(m.x, m.h_prev, m.w_ih, m.w_hh)) return false;
        if (split_cell && (!gru_aligned16(m.h_out) || m.h_out == m.h_prev || m.h_out == m.x)) return false;
    }
    return true;
}
