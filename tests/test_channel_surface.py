"""The public surface of the channel classes, pinned across refactors of adfl_amd/Channel: where each class
lives (instances are pickled into Ray actors by module and name), its to_json, that the reference's home
``Channel.quant`` resolves every name, that an instance holds only its constructor's state, and that the
uni-directional channels take their uncompressed direction from the one mix-in. No GPU: nothing is encoded.

The names are the nine classes plus the two ``Hip*`` aliases ``adfl_amd.Channel`` exports."""
import importlib
import pickle

import pytest

from adfl_amd.Channel import _base, quant

C = importlib.import_module("adfl_amd.Channel")   # the package: adfl_amd.Channel, the attribute, is the class

QUANT, STOCH = "adfl_amd.Channel.quant", "adfl_amd.Channel.stoch"
# exported name -> (class name, module, instance state of cls(4))
SURFACE = {
    "SLQChannel": ("SLQChannel", QUANT, {"bits": 4}),
    "USLQChannel": ("USLQChannel", QUANT, {"bits": 4}),
    "PackedSLQChannel": ("PackedSLQChannel", QUANT, {"bits": 4}),
    "HipSLQChannel": ("SLQChannel", QUANT, {"bits": 4}),
    "HipUSLQChannel": ("USLQChannel", QUANT, {"bits": 4}),
    "QSGDChannel": ("QSGDChannel", STOCH, {"bits": 4, "levels": 15}),
    "UQSGDChannel": ("UQSGDChannel", STOCH, {"bits": 4, "levels": 15}),
    "RQSGDChannel": ("RQSGDChannel", STOCH, {"bits": 4, "levels": 15}),
    "URQSGDChannel": ("URQSGDChannel", STOCH, {"bits": 4, "levels": 15}),
    "CNATChannel": ("CNATChannel", STOCH, {"bits": 4, "levels": 15}),
    "UCNATChannel": ("UCNATChannel", STOCH, {"bits": 4, "levels": 15}),
}
UNI = ["USLQChannel", "UQSGDChannel", "URQSGDChannel", "UCNATChannel"]


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_class_home_json_and_pickle(name):
    cls_name, module, state = SURFACE[name]
    cls = getattr(C, name)
    assert getattr(quant, name) is cls                      # the reference keeps them all in quant.py
    assert (cls.__name__, cls.__module__) == (cls_name, module)
    ch = cls(4)
    assert ch.to_json() == {"name": cls_name, "bits": 4}
    assert ch.__dict__ == state
    back = pickle.loads(pickle.dumps(ch))
    assert type(back) is cls and back.__dict__ == state


@pytest.mark.parametrize("name", UNI)
def test_unidirectional_channels_share_the_mixin(name):
    cls = getattr(C, name)
    assert cls.on_server_send is _base._Unidirectional.on_server_send
    assert cls.on_client_receive is _base._Unidirectional.on_client_receive
    assert cls.on_client_send is _base._CodecChannel.on_client_send         # the compressed direction
    assert cls.on_server_receive is _base._CodecChannel.on_server_receive


def test_codec_classes_define_no_surface_of_their_own():
    from adfl_amd.Channel import stoch
    for cls in (quant.SLQChannel, stoch._StochChannel):
        for m in ("on_server_send", "on_server_receive", "on_client_send", "on_client_receive", "to_json", "_send"):
            assert m not in vars(cls), (cls.__name__, m)
