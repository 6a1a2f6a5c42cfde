"""KG over pending fantasies in the wide form (kg_pending=2; include/spx.h: option "kg_fantasies" = 2): what needs no GPU."""
import pytest

from spearmint_amd import engine
from spearmint_amd.chooser import GPEIChooser, GPEIOptChooser


@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_arguments(mod, tmp_path):
    ch = mod.init(str(tmp_path), "acq=KG,kg_pending=2,kg_scan=1,acq_par=1023,kg_points=observed")
    assert (ch.kg_pending, ch.kg_scan, ch.acq_par, ch.kg_points) == (2, 1, 1023.0, "observed")
    assert [mod.init(str(tmp_path), "acq=KG,kg_pending=%d" % v).kg_pending for v in (0, 1)] == [0, 1]
    for args in ("acq=KG,kg_pending=2", "acq=EI,kg_pending=2", "acq=KG,kg_scan=1,kg_pending=3", "acq=KG,kg_scan=1,kg_pending=-1"):
        with pytest.raises(ValueError) as ei:
            mod.init(str(tmp_path), args)
        assert "allowed" in str(ei.value) and "kg_pending" in str(ei.value), args


def test_the_library_takes_the_option_without_a_gpu():
    eng = engine.Engine(0)
    for value in (0, 1, 2, 0):
        eng.set_option("kg_fantasies", value)
    assert eng.stat("last_kg_fantasies") == 0 and eng.stat("last_kg_scan") == 0
    eng.close()
