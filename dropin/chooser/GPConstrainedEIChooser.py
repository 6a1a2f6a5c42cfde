"""Drop-in `chooser.GPConstrainedEIChooser`: same module name, same `init`/`next`, same
`chooser.GPConstrainedEIChooser.pkl` state file as the reference module it shadows
(spearmint/spearmint/chooser/GPConstrainedEIChooser.py); the EI grid runs on the GPU via libspx.so."""
from spearmint_amd import util as _util
from spearmint_amd.chooser import GPConstrainedEIChooser as _impl


class GPConstrainedEIChooser(_impl.GPConstrainedEIChooser):
    # defined here so that self.__module__ == "chooser.GPConstrainedEIChooser", which names the
    # state pickle exactly as the reference does (GPConstrainedEIChooser.py: state_pkl)
    pass


def init(expt_dir, arg_string):
    return GPConstrainedEIChooser(expt_dir, **_util.unpack_args(arg_string))
