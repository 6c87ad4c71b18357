"""Which translation unit of libfreud_sae.so owns a kernel header (freud_amd/csrc/Makefile: SRCS, HDRS_<unit>).

A header that defines a non-template kernel must be compiled into exactly one unit -- every unit carries its own gfx950 code
object -- and that unit's object must be rebuilt when the header changes."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "freud_amd", "csrc")


def _make_var(makefile, name):
    m = re.search(r"^" + re.escape(name) + r"\s*:=\s*(.*)$", makefile, flags=re.M)
    assert m, f"the Makefile sets no {name}"
    return m.group(1).split()


def assert_one_unit_builds(header):
    """Exactly one unit of the Makefile's SRCS includes `header`, and the Makefile makes that unit's object depend on it.
    Returns the unit's file name."""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    units = _make_var(makefile, "SRCS")
    assert units and all(u.endswith(".hip") for u in units), units
    owners = [u for u in units if f'#include "{header}"' in open(os.path.join(CSRC, u)).read()]
    assert len(owners) == 1, f"{header} is included by {owners or 'no unit'} of {units}: exactly one must"
    stem = owners[0][:-len(".hip")]
    assert header in _make_var(makefile, f"HDRS_{stem}"), f"HDRS_{stem} does not list {header}"
    assert re.search(r"^\$\(OBJDIR\)/" + re.escape(stem) + r"\.o:\s*\$\(HDRS_" + re.escape(stem) + r"\)\s*$", makefile, flags=re.M), \
        f"the object of {owners[0]} does not depend on HDRS_{stem}"
    for other in units:
        if other != owners[0]:
            assert header not in _make_var(makefile, f"HDRS_{other[:-len('.hip')]}"), f"{other} does not include {header} but depends on it"
    return owners[0]
