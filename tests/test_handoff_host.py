"""CPU suite: the hand-off from the intersection pass to the pooling, as Python states it — the mirrors of the header's
constants, the test helper that packs a slot record, and the schedule's rule (``ops.sched_groups`` / ``ops.sched_words``).
No GPU, no library call."""
import pytest

from ocn_amd import ops
from tests.helpers import header_defines, slot_record, slot_record_fields


def test_python_mirrors_equal_the_header():
    d = header_defines()
    assert ops.SCHED_GROUP == d["OCN_SCHED_GROUP"]
    assert ops.SCHED_EIGHTHS == d["OCN_SCHED_EIGHTHS"] and ops.SCHED_MAX_EIGHTH == d["OCN_SCHED_MAX_EIGHTH"]
    assert ops.REC_WORDS == d["OCN_REC_WORDS"]
    assert ops.CLASS_RANGES == d["OCN_CLASS_RANGES"]
    assert ops.ST_CAP == d["OCN_ST_CAP"] and ops.ST_SCAN == d["OCN_ST_SCAN"]
    # the record's bits, as the header documents them: three distinct flags above a 61-bit offset, a 40-bit row start
    assert (d["OCN_REC_LEN_SHIFT"], d["OCN_REC_FULL2_BIT"], d["OCN_REC_HAS1_BIT"], d["OCN_REC_HAS2_BIT"]) == (40, 61, 62, 63)


EXTREME = dict(e=(1 << 21) - 1, i=(1 << 31) - 1, j=(1 << 31) - 1, a0=(1 << 40) - 1, da=1 << 21, base=1 << 40)


@pytest.mark.parametrize("flags", [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                                   (True, True, True)], ids=["none", "has1", "has2", "full2", "all"])
@pytest.mark.parametrize("low", [None, "i", "j", "a0", "da", "base"])
def test_slot_record_round_trip_at_the_field_extremes(flags, low):
    """Every field at its largest value (``low``: that one at zero instead, so that a neighbour's overflow into it shows),
    each flag alone: unpack(pack(x)) == x, the words are int64, and a flag moves exactly its own bit of word 3."""
    f = dict(EXTREME)
    if low:
        f[low] = 0
    has1, has2, full2 = flags
    words = slot_record(f["e"], f["i"], f["j"], f["a0"], f["da"], f["base"], has1, has2, full2)
    assert len(words) == 4 and all(-(1 << 63) <= w < (1 << 63) for w in words)
    assert slot_record_fields(words) == (f["e"], f["i"], f["j"], f["a0"], f["da"], f["base"], has1, has2, full2)
    bare = slot_record(f["e"], f["i"], f["j"], f["a0"], f["da"], f["base"], False, False, False)
    assert words[:3] == bare[:3] and bare[3] == f["base"]
    d = header_defines()
    assert (words[3] ^ bare[3]) & ((1 << 64) - 1) == (int(full2) << d["OCN_REC_FULL2_BIT"]) | (int(has1) << d["OCN_REC_HAS1_BIT"]) | (
        int(has2) << d["OCN_REC_HAS2_BIT"])
    assert (words[3] < 0) == has2                  # bit 63 of the unsigned word is the sign of the int64


# B -> groups at H = 256, as the three copies of the rule gave them before they became ops.sched_groups
GROUPS_256 = {0: 0, 4: 0, 28: 0, 32: 8, 36: 0, 64: 16, 2097120: 524280}


def test_sched_groups_and_words():
    for B, n in GROUPS_256.items():
        assert ops.sched_groups(B, 256) == n, B
        assert ops.sched_groups(B, 128) == 0, B
    assert ops.sched_groups(2097120 + 32, 256) == 0            # one group per eighth too many for 16-bit ranks
    assert [ops.sched_words(B) for B in GROUPS_256] == [0, 2, 14, 16, 18, 32, 1048560]
    assert [ops.sched_words(B) for B in (1, 3, 5, 61)] == [2, 2, 4, 32]      # 2 * ceil(B / 4)
