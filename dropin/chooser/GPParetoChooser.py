"""Drop-in `chooser.GPParetoChooser`: value against run time by expected hypervolume improvement on the GPU via libspx.so
(spearmint_amd/chooser/GPParetoChooser.py).  The reference has no module of this name; the shim follows the others so that
`--method=GPParetoChooser` works and the state file is `chooser.GPParetoChooser.pkl`."""
from spearmint_amd import util as _util
from spearmint_amd.chooser import GPParetoChooser as _impl


class GPParetoChooser(_impl.GPParetoChooser):
    # defined here so that self.__module__ == "chooser.GPParetoChooser" names the state pickle as the other shims do
    pass


def init(expt_dir, arg_string):
    return GPParetoChooser(expt_dir, **_util.unpack_args(arg_string))
