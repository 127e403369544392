"""contrastboundary_amd: hand-written HIP (gfx950) behind the reference's Python API.  The submodules are imported where they are used; the package itself
re-exports only the deterministic-training switch (neighbor_state.py), resolved on first use so that importing the package stays free of torch."""


def __getattr__(name):
    if name in ("deterministic", "set_deterministic", "is_deterministic"):
        from . import neighbor_state
        return getattr(neighbor_state, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
