"""CPU tests of the channel squelch's definition (tests/squelch_model.py; no GPU): the sequential rule on hand-written sequences, branch by branch, and the
proof that the scan form the kernel runs (three integer max-scans seeded from the carried state) gives the rule's mask and state on seeded random
class sequences, for every hang and from every carried state.  (The device is held to the model, in bytes, by tests/test_squelch_gpu.py.)"""
import numpy as np
import pytest

import squelch_model as S

INF, NAN = np.float32(np.inf), np.float32(np.nan)


def run(p, hang, open_thr=10.0, close_thr=4.0, gain=None, state=None):
    """one channel: the mask as a list and the state as a tuple"""
    mask, st = S.squelch(np.asarray(p, np.float32).reshape(-1, 1), None if gain is None else [gain], [open_thr], [close_thr], hang,
                         None if state is None else [state])
    return mask[:, 0].tolist(), tuple(int(v) for v in st[0])


def test_each_branch_of_the_rule():
    # closed stays closed below the open threshold, whatever the close threshold says
    assert run([0, 5, 9.999, 4], 3) == ([0, 0, 0, 0], (0, 0))
    # a strong block opens and loads the hang count; middle blocks reload it; low blocks count it down; the (hang + 1)-th low block closes
    assert run([10, 0, 0, 5, 0, 0, 0], 2) == ([1, 1, 1, 1, 1, 1, 0], (0, 0))
    assert run([10, 0, 0], 2) == ([1, 1, 1], (1, 0))
    assert run([10, 0], 2) == ([1, 1], (1, 1))
    assert run([10, 5], 2) == ([1, 1], (1, 2))
    # a middle block does not open a closed channel, a strong one reopens it
    assert run([10, 0, 0, 0, 5, 5, 10, 0], 2) == ([1, 1, 1, 0, 0, 0, 1, 1], (1, 1))
    # hang = 0: the first low block closes
    assert run([10, 5, 0, 5, 10, 0], 0) == ([1, 1, 0, 0, 1, 0], (0, 0))
    # equality at either threshold counts as reaching it
    assert run([10, 4, 3.9999998], 0) == ([1, 1, 0], (0, 0))
    assert run([np.nextafter(np.float32(10), np.float32(0)), 10], 0) == ([0, 1], (1, 0))


def test_powers_that_are_not_finite():
    # NaN is below both thresholds; +Inf is strong; -Inf is low
    assert run([NAN, 10, NAN, NAN], 1) == ([0, 1, 1, 0], (0, 0))
    assert run([INF, -INF, -INF], 1) == ([1, 1, 0], (0, 0))
    assert run([INF, NAN, 5], 5) == ([1, 1, 1], (1, 5))


def test_the_gain_scales_the_thresholds():
    # g2 = f32(g g): the thresholds follow the gained power, each product rounded once
    g = np.float32(3.0)
    p = (np.array([10, 5, 3.9, 10, 0], np.float32) * (g * g)).astype(np.float32)
    assert run(p, 0, gain=g) == run([10, 5, 3.9, 10, 0], 0)
    To, Tc = S.thresholds([0.1], [10.0], [4.0])
    assert To[0] == np.float32(np.float32(0.1) * np.float32(0.1)) * np.float32(10.0) and Tc.dtype == np.float32
    # gain 0: both products are +0, so every power >= 0 is strong, and a NaN power is not: the levels of a zeroed channel are +0, which opens at
    # thresholds of 0 only ... with thresholds above 0 the products are still 0
    assert run([0, 1, NAN, -1.0], 0, gain=0.0) == ([1, 1, 0, 0], (0, 0))
    # a g2 that overflows: To = Inf (only an infinite power is strong), and with a close threshold of 0 Tc = Inf * 0 = NaN, below which everything is
    assert run([1e38, INF, 1e38, INF], 0, open_thr=1.0, close_thr=0.0, gain=1e30) == ([0, 1, 0, 1], (1, 0))
    assert run([INF, INF], 1, open_thr=0.0, close_thr=0.0, gain=1e30) == ([0, 0], (0, 0))       # both products NaN: never open
    strong, low = S.classes(np.array([[INF]], np.float32), [1e30], [1.0], [0.0])
    assert strong[0, 0] and not low[0, 0]                 # strong goes first: a block is never both


def test_the_state_is_read_clamped():
    assert run([0, 0, 0], 5, state=(1, 2)) == ([1, 1, 0], (0, 0))
    assert run([0, 0, 0], 1, state=(1, 5)) == ([1, 0, 0], (0, 0))          # a smaller hang clamps h
    assert run([0], 5, state=(7, -3)) == ([0], (0, 0))                      # open is != 0, h at least 0
    assert run([0, 5], 5, state=(0, 4)) == ([0, 0], (0, 0))                 # a closed state carries no h
    assert run([], 3, state=(1, 9)) == ([], (1, 3))
    assert run([5, 0], 3, state=(1, 0)) == ([1, 1], (1, 2))


def test_calls_link_by_the_stream_position():
    rng = np.random.default_rng(3)
    p = rng.choice(np.array([0, 5, 10], np.float32), size=(40, 3), p=[0.6, 0.2, 0.2])
    whole, _ = S.squelch(p, None, [10.0] * 3, [4.0] * 3, 2)
    st = S.Stream(3)
    parts = [st.call(b0, p[b0:b1], None, [10.0] * 3, [4.0] * 3, 2) for b0, b1 in ((0, 7), (7, 8), (8, 29), (29, 40))]
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    again = st.call(29, p[29:], None, [10.0] * 3, [4.0] * 3, 2)            # elsewhere in the stream: closed in front
    assert again.tobytes() == S.squelch(p[29:], None, [10.0] * 3, [4.0] * 3, 2)[0].tobytes()


HANGS = (0, 1, 2, 5, 400)


def carried_states(hang):
    """closed, and open with every h for the small hangs; for the hang longer than the sequences both ends, the middle and the values around the
    sequence lengths"""
    hs = range(hang + 1) if hang <= 5 else sorted({0, 1, 2, 63, 64, 65, hang // 2, 299, 300, 301, hang - 1, hang})
    return [(0, 0)] + [(1, h) for h in hs]


@pytest.mark.parametrize("hang", HANGS)
def test_the_scan_form_is_the_sequential_rule(hang):
    """seeded class sequences (mostly low, so that runs of every length occur; some mostly middle; some all of one class), lengths 0 .. 300, every
    carried state: mask and state byte for byte"""
    rng = np.random.default_rng(100 + hang)
    for M in (0, 1, 2, 3, 7, 64, 65, 300):
        for probs in ((0.8, 0.15, 0.05), (0.5, 0.4, 0.1), (0.95, 0.04, 0.01), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            cls = rng.choice(3, size=(M, 6), p=probs)                       # 0 low, 1 middle, 2 strong
            strong, low = cls == 2, cls == 0
            for state in carried_states(hang):
                st = [state] * 6
                m1, s1 = S.run_classes(strong, low, hang, st)
                m2, s2 = S.scan_classes(strong, low, hang, st)
                assert m1.tobytes() == m2.tobytes(), (hang, M, probs, state)
                assert s1.tobytes() == s2.tobytes(), (hang, M, probs, state, s1.tolist(), s2.tolist())
    assert m1.dtype == np.uint8 and s1.dtype == np.int32 and s1.shape == (6, 2)


def test_the_scan_form_in_pieces():
    """the scan form carried from piece to piece (the kernel's chunks and the handle's calls) is the rule over the whole"""
    rng = np.random.default_rng(9)
    cls = rng.choice(3, size=(500, 4), p=(0.85, 0.1, 0.05))
    strong, low = cls == 2, cls == 0
    for hang in HANGS:
        whole, end = S.run_classes(strong, low, hang)
        st, parts = None, []
        for b0, b1 in ((0, 1), (1, 64), (64, 65), (65, 257), (257, 500)):
            m, st = S.scan_classes(strong[b0:b1], low[b0:b1], hang, st)
            parts.append(m)
        assert np.concatenate(parts).tobytes() == whole.tobytes() and st.tobytes() == end.tobytes()
        assert whole.any() and not whole.all()


def test_thresholds_from_db():
    o, c = S.db_thresholds([128, 256], -20.0, -23.0)
    assert o.dtype == np.float32 and np.allclose(o, [1.28, 2.56]) and np.allclose(c / o, 10 ** -0.3)
    o2, c2 = S.db_thresholds([128, 256], [-20.0, -10.0])
    assert o2.tobytes() == c2.tobytes() and np.allclose(o2, [1.28, 25.6])
