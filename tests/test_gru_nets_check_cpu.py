"""The refusal tables of the multi-net GRU entry points (csrc/gru_nets_check.hpp): ONE table of bad calls per record type, fed to the
fp32 route and to the split-bf16 route alike -- gru_seq_fwd_multi / gru_seq_split_fwd_multi, gru_seq_bwd_multi /
gru_seq_split_bwd_multi, gru_cell_fwd_multi / gru_cell_split_fwd_multi.  Every row is a valid call changed in one respect and must
come back as MO_ERR_BAD_ARG.  A refused call returns before any device call and dereferences no record pointer, so the records hold
made-up 16-byte aligned addresses and no GPU is needed; for the same reason no valid call is made here (it would launch) -- the GPU
suite makes those through the same ops.GruSeqNet / GruSeqBwdNet / GruCellNet structures.  The bad record is the last of two, so a
refusal also shows that the loop over the records reaches it."""
import ctypes as C
import functools

import pytest

from distributed_multi_agent_reinforcement_learning_amd import ops

BAD_ARG = 20001                    # include/mappo_ops.h MO_ERR_BAD_ARG
MAX_NETS, CELL_MAX_NETS = 24, 4    # include/mappo_ops.h MO_GRU_MAX_NETS, MO_GRU_CELL_MAX_NETS

SEQ_FWD = ("gi", "w_hh", "b_hh", "h0", "out", "save")
SEQ_FWD_REQUIRED = ("gi", "w_hh", "b_hh", "h0", "out")                      # save NULL: no backward
SEQ_FWD_ALIGNED = SEQ_FWD
SEQ_BWD = ("dout", "save", "out", "h0", "w_hh", "dgi", "dgh", "dnr", "dh0", "db_ih", "db_hh", "workspace")
SEQ_BWD_REQUIRED = ("dout", "save", "out", "h0", "w_hh", "dgi", "dh0")
SEQ_BWD_ALIGNED = ("dout", "save", "out", "h0", "dgi", "dgh", "dnr", "dh0", "workspace")
CELL = ("x", "h_prev", "w_ih", "w_hh", "b_ih", "b_hh", "h_out")
CELL_ALIGNED = ("x", "h_prev", "w_ih", "w_hh")                              # the fp32 cell; the split cell adds h_out


def _addr(fields, name):
    return 0x1000 * (1 + fields.index(name))


def _seq_fwd_net(B, **changed):
    return {**{f: _addr(SEQ_FWD, f) for f in SEQ_FWD}, "B": B, **changed}


def _seq_bwd_net(B, form="dnr", **changed):
    """a valid backward record in the dnr form (time-major dgi) or the dgh form, with both bias sums and their workspace"""
    net = {f: _addr(SEQ_BWD, f) for f in SEQ_BWD}
    net["dgh" if form == "dnr" else "dnr"] = None
    return {**net, "B": B, **changed}


def _cell_net(**changed):
    return {**{f: _addr(CELL, f) for f in CELL}, **changed}


def _array(struct, nets):
    arr = (struct * len(nets))()
    for a, net in zip(arr, nets):
        for name, value in net.items():
            setattr(a, name, value)
    return arr


SCALARS = dict(T=2, B=16, H=128, agents=0)


def _scalar_rows(good, max_nets, seq):
    """(label, n_nets, records or None, scalars): the rows that do not depend on the record type"""
    rows = [("n_nets 0", 0, [good], {}), (f"n_nets {max_nets + 1}", max_nets + 1, [good] * (max_nets + 1), {}), ("nets NULL", 2, None, {}),
            ("B 0", 2, [good, good], dict(B=0)), ("H 64", 2, [good, good], dict(H=64))]
    if seq:
        rows += [("T 0", 2, [good, good], dict(T=0)), ("gi_agents -1", 2, [good, good], dict(agents=-1)),
                 ("B 16, gi_agents 3", 2, [good, good], dict(agents=3))]
    return rows


def _record_rows(make, required, aligned):
    """(label, records, scalars): a good record first, then the record that is wrong in one field"""
    rows = [(f"{f} NULL", [make(16), make(16, **{f: None})], {}) for f in required]
    rows += [(f"{f} + 4", [make(16), make(16, **{f: make(16)[f] + 4})], {}) for f in aligned if make(16)[f] is not None]
    rows += [("m.B > B", [make(16), make(17)], {}), ("m.B < 0", [make(16), make(-1)], {}),
             ("m.B 16, gi_agents 3", [make(48), make(16)], dict(B=48, agents=3))]
    return rows


def _seq_bwd_rows():
    rows = _record_rows(_seq_bwd_net, SEQ_BWD_REQUIRED, SEQ_BWD_ALIGNED)
    dgh = functools.partial(_seq_bwd_net, form="dgh")                        # the other form: reaches dgh + 4
    rows += [(f"dgh form, {label}", nets, sc) for label, nets, sc in _record_rows(dgh, SEQ_BWD_REQUIRED, SEQ_BWD_ALIGNED)]
    good = _seq_bwd_net(16)
    rows += [("dgh and dnr", [good, _seq_bwd_net(16, dgh=_addr(SEQ_BWD, "dgh"))], {}), ("neither dgh nor dnr", [good, _seq_bwd_net(16, dnr=None)], {}),
             ("db_ih without db_hh", [good, _seq_bwd_net(16, db_hh=None)], {}), ("db_hh without db_ih", [good, _seq_bwd_net(16, db_ih=None)], {}),
             ("db_ih, db_hh without workspace", [good, _seq_bwd_net(16, workspace=None)], {})]
    return rows


def _call_seq(fn, struct, n, nets, sc):
    sc = {**SCALARS, **sc}
    arr = None if nets is None else C.cast(_array(struct, nets), C.c_void_p)
    return fn(n, arr, sc["T"], sc["B"], sc["H"], sc["agents"], None)


@pytest.mark.parametrize("entry", ["gru_seq_fwd_multi", "gru_seq_split_fwd_multi", "gru_seq_bwd_multi", "gru_seq_split_bwd_multi"])
def test_sequence_entry_points_refuse_every_row(entry):
    fn = getattr(ops.load_library(), entry)
    bwd = "bwd" in entry
    struct, good = (ops.GruSeqBwdNet, _seq_bwd_net(16)) if bwd else (ops.GruSeqNet, _seq_fwd_net(16))
    rows = [(label, n, nets, sc) for label, n, nets, sc in _scalar_rows(good, MAX_NETS, seq=True)]
    rows += [(label, 2, nets, sc) for label, nets, sc in (_seq_bwd_rows() if bwd else _record_rows(_seq_fwd_net, SEQ_FWD_REQUIRED, SEQ_FWD_ALIGNED))]
    assert len({label for label, *_ in rows}) == len(rows) == (8 + 5 + 6 + 3 if not bwd else 8 + 2 * (7 + 8 + 3) + 5)
    for label, n, nets, sc in rows:
        assert _call_seq(fn, struct, n, nets, sc) == BAD_ARG, (entry, label)


@pytest.mark.parametrize("entry", ["gru_cell_fwd_multi", "gru_cell_split_fwd_multi"])
def test_cell_entry_points_refuse_every_row(entry):
    fn = getattr(ops.load_library(), entry)
    good = _cell_net()
    rows = _scalar_rows(good, CELL_MAX_NETS, seq=False)
    rows += [(f"{f} NULL", 2, [good, _cell_net(**{f: None})], {}) for f in CELL]
    rows += [(f"{f} + 4", 2, [good, _cell_net(**{f: good[f] + 4})], {}) for f in CELL_ALIGNED]
    if entry == "gru_cell_split_fwd_multi":    # two workgroups share a row tile and store 16 bytes at a time: not in place, aligned
        rows += [("h_out == h_prev", 2, [good, _cell_net(h_out=good["h_prev"])], {}), ("h_out == x", 2, [good, _cell_net(h_out=good["x"])], {}),
                 ("h_out + 4", 2, [good, _cell_net(h_out=good["h_out"] + 4)], {})]
    assert len(rows) == 5 + 7 + 4 + 3 * (entry == "gru_cell_split_fwd_multi")
    for label, n, nets, sc in rows:
        sc = {**SCALARS, **sc}
        arr = None if nets is None else C.cast(_array(ops.GruCellNet, nets), C.c_void_p)
        assert fn(n, arr, sc["B"], sc["H"], None) == BAD_ARG, (entry, label)
