"""Host-side mirrors of the reference's hot-path nn.Module classes (same constructor / forward
signatures and state_dict keys); arithmetic runs in libcvc_hip.so."""


def __getattr__(name):
    # cvc.model.CaptionEnsemble, resolved on first use (the package itself imports nothing)
    if name == "CaptionEnsemble":
        from .ensemble import CaptionEnsemble
        return CaptionEnsemble
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
