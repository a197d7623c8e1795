"""CPU tests of the tone squelch's definition (tests/tone_squelch_model.py; no GPU): the frame class branch by branch on hand-made rows, the scan form
the kernel runs against the sequential rule, the causal expansion against a double loop, every cut of a stream equal to the uncut stream, and the
restart at a gap.  (The host side: tests/test_tone_squelch_api_cpu.py; the device against this model, in bytes: tests/test_tone_squelch_gpu.py.)"""
import numpy as np
import pytest

import tone_squelch_model as M

F32 = np.float32
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def row(*mags):
    """a row whose e_t are exactly the given float32 values where they are squares of float32 (the magnitude goes into re)"""
    z = np.zeros(len(mags), np.complex64)
    z.real = np.asarray(mags, np.float32)
    return z


def cls(r, sel, o, c, ratio=0.0, guard=0):
    s, low = M.frame_class(r, sel, F32(o), F32(c), F32(ratio), guard)[:2]
    return "strong" if s else "low" if low else "hold"


def test_energy_is_two_rounded_products_and_a_rounded_sum():
    z = np.array([np.float32(1.0000001) + 1j * np.float32(3.0000002)], np.complex64)
    re, im = z.real.astype(np.float32)[0], z.imag.astype(np.float32)[0]
    want = F32(F32(re * re) + F32(im * im))
    assert M.energies(z)[0] == want and M.energies(z).dtype == np.float32
    assert M.energies(row(2.0, 0.0, 3.0)).tolist() == [4.0, 0.0, 9.0]


def test_thresholds_with_equality():
    r = row(2.0, 0.0)                                                     # e = 4
    assert cls(r, 0, 4.0, 1.0) == "strong"                                # e == open: >= holds
    assert cls(r, 0, np.nextafter(F32(4), INF), 4.0) == "hold"            # just below open, e == close
    assert cls(r, 0, 8.0, np.nextafter(F32(4), INF)) == "low"             # just below close
    assert cls(r, 0, 0.0, 0.0) == "strong" and cls(row(0.0, 0.0), 0, 0.0, 0.0) == "strong"     # thresholds of 0: +0 reaches them


def test_the_ratio_with_equality_and_ratio_zero():
    r = row(2.0, 1.0, 0.5)                                                # e = 4, others 1 and 0.25: o = 1
    assert M.frame_class(r, 0, F32(1), F32(1), F32(0), 0)[3] == F32(1.0)
    assert cls(r, 0, 1.0, 1.0, ratio=4.0) == "strong"                     # e == R
    assert cls(r, 0, 1.0, 1.0, ratio=np.nextafter(F32(4), INF)) == "low"  # e just below R: neither strong nor hold
    assert cls(r, 0, 8.0, 1.0, ratio=4.0) == "hold" and cls(r, 0, 8.0, 1.0, ratio=4.5) == "low"
    assert cls(row(2.0, 1e18), 0, 1.0, 1.0, ratio=0.0) == "strong"        # ratio 0: R = +0 whatever the others are (finite)
    # the product is rounded to float32 once
    o = M.frame_class(row(2.0, 1.1), 0, F32(1), F32(1), F32(0), 0)[3]
    R = F32(F32(3.3) * o)
    e = F32(4.0)
    assert cls(row(2.0, 1.1), 0, 1.0, 1.0, ratio=3.3) == ("strong" if e >= R else "low")


def test_nan_and_inf_in_the_selected_tone():
    assert cls(row(NAN, 1.0), 0, 0.0, 0.0) == "low"                       # NaN is below every threshold, +0 included
    z = np.array([complex(0.0, np.nan), 1.0], np.complex64)
    assert cls(z, 0, 0.0, 0.0) == "low"
    assert cls(row(INF, 1.0), 0, 1e30, 1.0, ratio=1e30) == "strong"       # Inf >= anything finite
    assert cls(row(INF, 1.0), 0, 1.0, 1.0, ratio=0.0) == "strong"
    assert cls(row(-INF, 1.0), 0, 1.0, 1.0) == "strong"                   # (-Inf)^2 = +Inf
    assert cls(row(1e30, 1.0), 0, 1.0, 1.0) == "strong"                   # the product overflows to +Inf


def test_nan_and_inf_in_the_other_tones():
    assert M.frame_class(row(2.0, NAN, 1.0), 0, F32(1), F32(1), F32(1), 0)[3] == F32(1.0)    # a NaN is never taken, in any place
    assert M.frame_class(row(2.0, 1.0, NAN), 0, F32(1), F32(1), F32(1), 0)[3] == F32(1.0)
    assert M.frame_class(row(2.0, NAN, NAN), 0, F32(1), F32(1), F32(1), 0)[3] == F32(0.0)
    assert cls(row(2.0, NAN, 1.0), 0, 1.0, 1.0, ratio=4.0) == "strong"
    assert cls(row(2.0, INF), 0, 1.0, 1.0, ratio=1.0) == "low"            # o = Inf, R = Inf
    assert cls(row(2.0, INF), 0, 1.0, 1.0, ratio=0.0) == "low"            # 0 Inf = NaN: nothing reaches it
    assert cls(row(INF, INF), 0, 1.0, 1.0, ratio=1.0) == "strong"         # Inf >= Inf


def test_the_guard_at_both_ends_and_beyond():
    r = row(2.0, 3.0, 4.0, 5.0, 6.0)                                      # e_t = 4 9 16 25 36
    o = lambda sel, g: float(M.frame_class(r, sel, F32(0), F32(0), F32(0), g)[3])
    assert [o(0, g) for g in range(6)] == [36.0, 36.0, 36.0, 36.0, 0.0, 0.0]        # sel = 0: guard 4 leaves none
    assert [o(4, g) for g in range(6)] == [25.0, 16.0, 9.0, 4.0, 0.0, 0.0]          # sel = T - 1
    assert [o(2, g) for g in range(4)] == [36.0, 36.0, 0.0, 0.0]
    assert cls(r, 0, 1.0, 1.0, ratio=1e30, guard=63) == "strong"          # guard >= T: o = +0, R = +0
    assert cls(row(2.0), 0, 1.0, 1.0, ratio=1e30, guard=0) == "strong"    # T = 1 likewise


def test_a_channel_without_a_tone():
    Z = np.zeros((3, 2, 2), np.complex64)
    Z[:, 1, 0] = 2.0
    dec, st = M.decide(Z, [-1, 0], [F32(1)] * 2, [F32(1)] * 2, [F32(0)] * 2, 0, 2, state=np.array([[1, 2], [0, 0]]))
    assert dec[:, 0].tolist() == [1, 1, 1] and st[0].tolist() == [0, 0]
    assert dec[:, 1].tolist() == [1, 1, 1] and st[1].tolist() == [1, 2]
    cm = np.array([[1, 1], [0, 1], [1, 0]], np.uint8)
    assert M.gate(cm, dec, [-1, 0], 1, 0, None)[:, 0].tolist() == [1, 0, 1]          # its carrier mask, even in front of the first frame
    assert M.gate(cm, dec, [-1, 0], 1, 0, None)[:, 1].tolist() == [0, 1, 0]
    dec0, st0 = M.decide(np.zeros((0, 2, 2), np.complex64), [-1, 0], [F32(1)] * 2, [F32(1)] * 2, [F32(0)] * 2, 0, 2, state=np.array([[1, 2], [1, 7]]))
    assert dec0.shape == (0, 2) and st0.tolist() == [[0, 0], [1, 2]]      # no frame: the state as it is READ (h clipped to the hang in force)


@pytest.mark.parametrize("hang", [0, 1, 3, 70])
def test_the_scan_form_is_the_sequential_rule(hang):
    rng = np.random.default_rng(hang)
    for nf in (1, 2, 63, 64, 65, 130):
        strong = rng.random((nf, 6)) < 0.15
        low = ~strong & (rng.random((nf, 6)) < 0.7)
        for state in (None, np.array([[1, h] for h in ([0, hang, hang // 2] * 2)]), np.array([[0, 0]] * 6)):
            a, b = M.run_classes(strong, low, hang, state), M.scan_classes(strong, low, hang, state)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


@pytest.mark.parametrize("W", [1, 2, 4, 9])
def test_the_causal_expansion_against_a_double_loop(W):
    rng = np.random.default_rng(W)
    C, nb = 3, 2 * W + 3
    for fill in range(W):
        nf = (fill + nb) // W
        dec = (rng.random((nf, C)) < 0.5).astype(np.uint8)
        cm = (rng.random((nb, C)) < 0.7).astype(np.uint8)
        st = np.array([[1, 0], [0, 0], [1, 1]])
        got = M.gate(cm, dec, [0, 0, 0], W, fill, st)
        # the double loop: frame by frame of the call, block by block inside it
        want = np.zeros_like(cm)
        m = 0
        for j in range(nf + 1):
            first = 0 if j else fill
            for _ in range(first, W):
                if m == nb:
                    break
                for c in range(C):
                    want[m, c] = cm[m, c] & (st[c, 0] if j == 0 else dec[j - 1, c])
                m += 1
        assert m == nb and (got == want).all()


def stream_case(W=2, T=4, C=3, NB=9, hang=1):
    rng = np.random.default_rng(7)
    nf = NB // W
    Z = (rng.standard_normal((nf, C, T)) + 1j * rng.standard_normal((nf, C, T))).astype(np.complex64)
    Z[:, :, 1] *= (rng.random((nf, C)) < 0.5) * 4.0
    cm = (rng.random((NB, C)) < 0.8).astype(np.uint8)
    setting = dict(tone=[1, 1, -1], open_thr=[F32(8)] * C, close_thr=[F32(2)] * C, ratio=[F32(1.5)] * C, guard=0, hang=hang)
    return Z, cm, setting


def run_cut(Z, cm, setting, W, cut, first=0):
    s = M.Stream(cm.shape[1], W)
    decs, masks, b, f = [], [], 0, 0
    for n in cut:
        nf = ((s.fill if first + b == s.next else 0) + n) // W
        d, m = s.call(first + b, Z[f:f + nf], cm[b:b + n], **setting)
        decs.append(d)
        masks.append(m)
        b, f = b + n, f + nf
    return np.concatenate(decs), np.concatenate(masks)


def test_all_256_cuts_of_a_nine_block_stream():
    for W in (1, 2, 4):
        Z, cm, setting = stream_case(W=W)
        dec0, mask0 = run_cut(Z, cm, setting, W, [9])
        assert dec0.shape[0] == 9 // W and set(dec0[:, :2].ravel().tolist()) == {0, 1}          # (the case decides both ways)
        assert (mask0[:W, :2] == 0).all()                                 # the first frame of a fresh stream is closed
        assert (mask0[:, 2] == cm[:, 2]).all()
        for bits in range(256):
            cut, n = [], 1
            for k in range(8):
                if bits >> k & 1:
                    cut.append(n)
                    n = 1
                else:
                    n += 1
            cut.append(n)
            assert sum(cut) == 9
            dec, mask = run_cut(Z, cm, setting, W, cut)
            assert (dec == dec0).all() and (mask == mask0).all(), (W, cut)


def test_restart_at_a_gap_and_at_a_new_setting():
    W = 2
    Z, cm, setting = stream_case(W=W, NB=8)
    Z[:] = 0
    Z[:, :, 1] = 3.0                                                      # every frame strong: open from frame 0 on
    s = M.Stream(3, W)
    d, m = s.call(0, Z[:2], cm[:4], **setting)
    assert (d[:, :2] == 1).all() and (m[:2, :2] == 0).all() and (m[2:, :2] == cm[2:4, :2]).all()
    d, m = s.call(4, Z[2:3], cm[4:6], **setting)                          # continues: the carried open state is in force at once
    assert (m[:, :2] == cm[4:6, :2]).all()
    d, m = s.call(7, Z[3:3], cm[7:8], **setting)                          # a gap: (0, 0) and fill 0
    assert d.shape[0] == 0 and (m[:, :2] == 0).all() and s.fill == 1
    s = M.Stream(3, W)
    s.call(0, Z[:1], cm[:3], **setting)                                   # fill 1 behind it
    s.restart()                                                           # a new setting: the state only
    assert s.fill == 1
    d, m = s.call(3, Z[1:3], cm[3:6], **setting)
    assert d.shape[0] == 2 and (m[:1, :2] == 0).all() and (m[1:, :2] == cm[4:6, :2]).all()


def test_hang_counts_frames():
    Z = np.zeros((6, 1, 2), np.complex64)
    Z[0, 0, 0] = 3.0
    for hang, want in ((0, [1, 0, 0, 0, 0, 0]), (1, [1, 1, 0, 0, 0, 0]), (3, [1, 1, 1, 1, 0, 0])):
        dec, st = M.decide(Z, [0], [F32(4)], [F32(1)], [F32(0)], 0, hang)
        assert dec[:, 0].tolist() == want and st.tolist() == [[0, 0]]
    dec, st = M.decide(Z[:3], [0], [F32(4)], [F32(1)], [F32(0)], 0, 3)
    assert st.tolist() == [[1, 1]]
    dec2, _ = M.decide(Z[3:], [0], [F32(4)], [F32(1)], [F32(0)], 0, 3, st)
    assert dec2[:, 0].tolist() == [1, 0, 0]
