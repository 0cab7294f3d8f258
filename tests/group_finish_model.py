"""
The forward subgrid side with the STRIDED axis finished first (csrc/swiftly_groupfinish.h), emulated on the CPU in the style
of tests/accuracy_model.py (test infrastructure; uses the oracle).

``forward_chain_group_finish`` replays one facet -> one subgrid through K1 and K2 exactly as ``accuracy_model.forward_chain``
does and then through the new order: the column kernel (m-point transform along axis 0, Fn, placement, xM-point inverse,
crop to xA rows -- nothing stored in between) writes ``T[xA, m]`` in complex64, the row kernel (the same along axis 1)
writes the subgrid.  Against the parent's order one stored intermediate fewer (G and the half-finished subgrid become T).

``subgrid_side`` is the same pair of steps for a whole wave of random K2 windows, summed over the facets of every off1 group
in the column step and over the groups in the row step, in float32 or float64 arithmetic: the model the GPU tests take
their margin from.
"""
import numpy

import accuracy_model as am
from oracle import swiftly_oracle as orc


def _finish_axis(c, x, facet_offs, sub_off, xA, axis, bits, dtype_w):
    """sum over ``x[n]`` of place(Fn * cfft_m(x[n], axis)) by ``facet_offs[n]``, xM-point inverse, crop to xA: one axis of
    add_to_subgrid + finish_subgrid (core.py:255-325) in ``bits`` arithmetic"""
    m, xM = c.xM_yN_size, c.xM_size
    k = numpy.arange(m)
    fn = c.Fn.astype(numpy.float32).astype(dtype_w)
    shape = list(x[0].shape)
    shape[axis] = xM
    acc = numpy.zeros(shape, dtype=numpy.complex64 if bits == 32 else numpy.complex128)
    for xn, off in zip(x, facet_offs):
        sp = c._sp(off)
        g = am._centred(xn, axis, bits, False)
        g = numpy.take(g, (k + sp) % m, axis=axis) * (fn[:, None] if axis == 0 else fn[None, :])
        idx = (k + xM // 2 - m // 2 + sp) % xM
        if axis == 0:
            acc[idx, :] += g.astype(acc.dtype)
        else:
            acc[:, idx] += g.astype(acc.dtype)
    i = numpy.arange(xA)
    return numpy.take(am._centred(acc, axis, bits, True), (xM // 2 - xA // 2 + i + sub_off) % xM, axis=axis)


def forward_chain_group_finish(P, facet, fo, so, bits, scratch_split=None, round_stores=True):
    """accuracy_model.forward_chain with the subgrid side in the new order.  bits = dict(k1=, k2=, k3=, sf=): ``k3`` is the
    arithmetic of the column kernel (it holds the m-point transform K3 used to run), ``sf`` that of the row kernel."""
    c = orc.OracleCore(P["W"], P["N"], P["xM"], P["yN"])
    yB, yN, xA, m = P["yB"], P["yN"], P["xA"], c.xM_yN_size
    rnd = am._c64 if round_stores else (lambda a: a)
    w = c.facet_window(yB).astype(numpy.float32)
    wt = {32: numpy.float32, 64: numpy.float64}
    y = numpy.arange(yB)
    pos = lambda off: (yN // 2 - yB // 2 + y + off) % yN  # noqa: E731
    t = bits["k1"]
    x = facet.astype(numpy.complex64 if t == 32 else numpy.complex128)
    x = x * w.astype(wt[t])[None, :] * w.astype(wt[t])[:, None]
    k1 = numpy.zeros((yB, yN), dtype=x.dtype)
    k1[:, pos(fo[1])] = x
    k1 = rnd(am._centred(k1, 1, t, True))
    t = bits["k2"]
    col = c.extract_from_facet(k1, so[1], 1)
    k2 = numpy.zeros((yN, m), dtype=col.dtype)
    k2[pos(fo[0]), :] = col
    k2 = am._centred(k2, 0, t, True, mid_round=scratch_split)
    q = rnd(c.extract_from_facet(k2, so[0], 0))                   # [m, m]
    t = bits["k3"]
    T = rnd(_finish_axis(c, [q], [fo[0]], so[0], xA, 0, t, wt[t]))  # [xA, m], stored in complex64
    t = bits["sf"]
    return rnd(_finish_axis(c, [T], [fo[1]], so[1], xA, 1, t, wt[t])).astype(complex)


def subgrid_side(c, windows, facet_offs, sub_off, xA, bits, mask0=None, mask1=None, stage=3, T=None):
    """The new subgrid side for one subgrid.  ``windows[f]`` = [m, m] K2 window of facet f (extract_from_facet along both
    axes), ``facet_offs[f]`` = (off0, off1), ``sub_off`` = (off0, off1).  Returns ``(T, out)``: T[g] = [xA, m] per off1 group
    in ascending off1 (complex64 values), out = [xA, xA].  ``stage`` 1 stops after T; 2 starts from the given ``T``."""
    wt = numpy.float32 if bits == 32 else numpy.float64
    groups = sorted({o[1] for o in facet_offs})
    if stage & 1:
        T = []
        for g1 in groups:
            members = [f for f, o in enumerate(facet_offs) if o[1] == g1]
            t = _finish_axis(c, [windows[f] for f in members], [facet_offs[f][0] for f in members], sub_off[0], xA, 0, bits, wt)
            if mask0 is not None:
                t = t * mask0.astype(wt)[:, None]
            T.append(am._c64(t))
    if not stage & 2:
        return T, None
    out = _finish_axis(c, list(T), groups, sub_off[1], xA, 1, bits, wt)
    if mask1 is not None:
        out = out * mask1.astype(wt)[None, :]
    return T, am._c64(out)
