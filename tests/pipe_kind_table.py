"""The Pipe kinds' numbers as saved states hold them, and the reader of the one kind table (sdr_amd/csrc/pipe.hpp) that the device-less
Pipe tests share.  TEST INFRASTRUCTURE ONLY."""
import os
import re

KIND_NUMBERS = {"PK_FILTER": 0, "PK_DECIMATOR": 1, "PK_RESAMPLER": 2, "PK_DEMOD": 3, "PK_DCBLOCK": 4, "PK_AGC": 5, "PK_TUNER": 6,
                "PK_TUNER_BANK": 7, "PK_AM": 8, "PK_AM_BANK": 9, "PK_SPECTRUM": 10, "PK_NFM_BANK": 11, "PK_AM_BANK_AUDIO": 12,
                "PK_NFM_BANK_AUDIO": 13, "PK_NARROW_BANK": 14}


def pipe_kind_table():
    """[(name, number)] of the one kind table, sdr_amd/csrc/pipe.hpp's `enum PipeKind`, in the order written: every kind is given its
    number explicitly (`NAME = N`), and no other definition of a kind stands anywhere in the Pipe layer's sources."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_amd", "csrc")
    src = open(os.path.join(csrc, "pipe.hpp")).read()
    bodies = re.findall(r"enum PipeKind : int \{(.*?)\};", src, re.S)
    assert len(bodies) == 1, "one enum PipeKind"
    items = [i.strip() for i in re.sub(r"//[^\n]*", "", bodies[0]).split(",")]
    table = []
    for item in filter(None, items):
        m = re.fullmatch(r"(PK_[A-Z0-9_]+) = (\d+)", item)
        assert m, f"`{item}`: every kind is written NAME = N"
        table.append((m.group(1), int(m.group(2))))
    for f in os.listdir(csrc):
        if f.startswith("pipe"):
            text = open(os.path.join(csrc, f)).read()
            assert not re.search(r"constexpr\s+PipeKind|static_cast<PipeKind>", text), f"{f} defines a kind outside the table"
    return table
