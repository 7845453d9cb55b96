"""CPU test of the rule that sorts the wavefronts of the 512 x 1 LP kernel into the classes its specialised PCG loops are compiled for
(lpbox_wave_class_rule, the function LpBatch.wave_classes applies to the layout): against a numpy restatement."""
import numpy as np
import pytest

CAPS = (12, 12, 8)          # register entries of a lane's row, own-column and helper list


def restated(lens):
    """lens: (3, lanes).  Chunks of two register entries of the longest list, per list; tail when a list exceeds its registers."""
    lens = np.asarray(lens).reshape(3, -1)
    cap = np.array(CAPS)[:, None]
    chunks = (np.minimum(lens, cap) + 1) // 2
    return tuple(int(v) for v in chunks.max(axis=1, initial=0)) + (int((lens > cap).any()),)


def cases():
    rs = np.random.RandomState(7)
    out = [np.zeros((3, 64), int), np.zeros((3, 0), int)]
    for cap_hit in range(3):                                  # exactly at a capacity, one beyond it, in one lane
        for extra in (0, 1):
            a = rs.randint(0, 5, (3, 64))
            a[cap_hit, rs.randint(64)] = CAPS[cap_hit] + extra
            out.append(a)
    for hi in (1, 2, 3, 9, 13, 30):                           # odd and even maxima, short and far beyond the registers
        out.append(rs.randint(0, hi + 1, (3, 64)))
    one = np.zeros((3, 64), int)
    one[1, 17] = 1                                            # a single lane with a single entry
    out.append(one)
    return out


@pytest.mark.parametrize("k", range(len(cases())))
def test_rule_matches_the_restatement(k):
    from lpbox_hip.lp import wave_class_rule
    a = cases()[k]
    assert wave_class_rule(a[0], a[1], a[2]) == restated(a)


def test_every_class_is_reached_and_bounded():
    from lpbox_hip.lp import wave_class_rule
    seen = set()
    for r in range(0, 14):
        for c in range(0, 14):
            for h in range(0, 10):
                got = wave_class_rule([r], [c], [h])
                assert got == restated([[r], [c], [h]])
                assert got[0] <= 6 and got[1] <= 6 and got[2] <= 4
                seen.add(got[:3])
    assert len(seen) == 7 * 7 * 5
