"""float64 restatement of the ML3Layer edge branch of include/gml.h (gml_edge_mlp_fwd / _fwd6 / _fwd_exact / the stacks, gml_edge_mlp_bwd
/ _bwd_exact / _bwd_sym, gml_edge_mlp_wide_fwd / _wide_bwd) with the TERM SUM of every element.  Plain numpy, no device, nothing
imported from the package: tests/test_edge_ref_cpu.py holds it to float64 autograd of oracle.spect_conv_oracle.edge_mlp_forward.

    z1 = W1 e, z2 = W2 e, z3 = W3 e          h = [relu(z1) ; tanh(z2) tanh(z3)]          o = W4 h          out = relu(o)
    go = gout (o > 0)                        dh = W4^T go
    dz1 = dh[:2S] (z1 > 0)                   dz2 = dh[2S:] tanh(z3) (1 - tanh(z2)^2)     dz3 = dh[2S:] tanh(z2) (1 - tanh(z3)^2)
    gin = W1^T dz1 + W2^T dz2 + W3^T dz3     dWm = sum_e dzm e^T  (m = 1, 2, 3)          dW4 = sum_e go h^T

relu'(0) = 0 (torch's convention).  Unique rows (uid, mir given): entry u evaluates edge uid[u] on the output gradient
gout[uid[u]] + gout[mir[u]] (mir[u] < 0: gout[uid[u]] alone), the weight gradients sum over the entries and there is no gin.

TERM SUM of an element: the same expression with every product replaced by the product of the absolute values of its factors and
every tanh and tanh' replaced by its bound 1 (the precedent: _conv_ref.mix_ref adds 1 for its tanh factors).  relu' stays the
reference's 0 / 1 pattern: an element the pattern closes has no terms and must be exactly zero -- the backward's inputs keep a
relu margin (oracle.relu_margin), so a correct kernel decides every pattern as the reference does.  The forward's own relus are
1-Lipschitz and carry no pattern: T(relu(z)) = T(z), so an output whose argument lies within rounding of zero may come out as a
rounding-sized positive number.  For dW the term sum is the sum over the edges of the absolute per-edge terms.  Written out:

    T(z1) = |W1| |e|                          T(h) = [T(z1) ; 1]                          T(out) = |W4| T(h)
    T(go) = |gout| (o > 0)  (unique rows: (|gout[uid]| + |gout[mir]|) (o > 0))            T(dh) = |W4|^T T(go)
    T(dz1) = T(dh)[:2S] (z1 > 0)              T(dz2) = T(dz3) = T(dh)[2S:]
    T(gin) = |W1|^T T(dz1) + |W2|^T T(dz2) + |W3|^T T(dz3)
    T(dWm) = sum_e T(dzm) |e|^T               T(dW4) = sum_e T(go) [T(z1) (z1 > 0) ; 1]^T

Why this definition: every T is >= the absolute value of its element, and tol T of an element that passes through a tanh is at
least tol |W4| resp. tol |dh|: far more than the short tanh's documented absolute error (2e-7, gml_tanh_short) carried through |W4|.
A correct kernel therefore cannot be failed by its tanh alone, while an element of small magnitude among large ones is still held
to its own terms instead of the tensor's maximum.

Every result is a _conv_ref.Ref(v, t, n): value, term sum, number of terms of the longest sum in the element (an fp32 bound's n)."""
import numpy as np

from _conv_ref import Ref


def _f64(*arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def _forward(ea, w1, w2, w3, w4):
    z1, z2, z3 = ea @ w1.T, ea @ w2.T, ea @ w3.T
    T1 = np.abs(ea) @ np.abs(w1).T
    t2, t3 = np.tanh(z2), np.tanh(z3)
    h = np.concatenate([np.maximum(z1, 0.0), t2 * t3], 1)
    o = h @ w4.T
    return z1, T1, t2, t3, h, o


def edge_fwd_ref(ea, w1, w2, w3, w4):
    """Ref of out [E, Sout].  ea [E, S], w1 .. w3 [2S, S], w4 [Sout, 4S]."""
    ea, w1, w2, w3, w4 = _f64(ea, w1, w2, w3, w4)
    z1, T1, t2, t3, h, o = _forward(ea, w1, w2, w3, w4)
    Th = np.concatenate([T1, np.ones_like(T1)], 1)
    S = ea.shape[1]
    return Ref(np.maximum(o, 0.0), Th @ np.abs(w4).T, float(4 * S + S))


def edge_bwd_ref(ea, w1, w2, w3, w4, gout, uid=None, mir=None, wide=False):
    """{'gin': Ref [E, S] (None with uid), 'dw1' .. 'dw3': Ref [2S, S], 'dw4': Ref [Sout, 4S]}; wide = True adds 'go' [E, Sout],
    'hid' [E, 2, 2S] and 'gz' [E, 3, 2S] as gml_edge_mlp_wide_bwd defines them (its rows pad each block to H2R columns)."""
    ea, w1, w2, w3, w4, gout = _f64(ea, w1, w2, w3, w4, gout)
    ag = np.abs(gout)
    if uid is not None:
        uid, mir = np.asarray(uid, np.int64), np.asarray(mir, np.int64)
        has = (mir >= 0)[:, None]
        m = np.where(mir >= 0, mir, 0)
        ea, gout, ag = ea[uid], gout[uid] + gout[m] * has, ag[uid] + ag[m] * has
    E, S = ea.shape
    z1, T1, t2, t3, h, o = _forward(ea, w1, w2, w3, w4)
    m1, mo = z1 > 0, o > 0
    go, Tgo = gout * mo, ag * mo
    dh, Tdh = go @ w4, Tgo @ np.abs(w4)
    H2 = 2 * S
    dz1, Tdz1 = dh[:, :H2] * m1, Tdh[:, :H2] * m1
    dz2, dz3 = dh[:, H2:] * t3 * (1 - t2 * t2), dh[:, H2:] * t2 * (1 - t3 * t3)
    Tdz2 = Tdz3 = Tdh[:, H2:]
    ae = np.abs(ea)
    Th = np.concatenate([T1 * m1, np.ones_like(T1)], 1)
    n = float(max(E, 1))
    r = {'gin': None if uid is not None else Ref(dz1 @ w1 + dz2 @ w2 + dz3 @ w3,
                                                 Tdz1 @ np.abs(w1) + Tdz2 @ np.abs(w2) + Tdz3 @ np.abs(w3), float(6 * S)),
         'dw1': Ref(dz1.T @ ea, Tdz1.T @ ae, n), 'dw2': Ref(dz2.T @ ea, Tdz2.T @ ae, n), 'dw3': Ref(dz3.T @ ea, Tdz3.T @ ae, n),
         'dw4': Ref(go.T @ h, Tgo.T @ Th, n)}
    if wide:
        r['go'] = Ref(go, Tgo, 1.0)
        r['hid'] = Ref(np.stack([h[:, :H2], h[:, H2:]], 1), np.stack([T1, np.ones_like(T1)], 1), float(S))
        r['gz'] = Ref(np.stack([dz1, dz2, dz3], 1), np.stack([Tdz1, Tdz2, Tdz3], 1), float(w4.shape[0]))
    return r
