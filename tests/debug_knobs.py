"""Context managers around the library's hz_debug_set knobs, shared by the GPU tests."""


class fast_cap:
    """hz_debug_set("shadow_fast_cap", n) for the block, the default restored afterwards."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"shadow_fast_cap", self.n))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"shadow_fast_cap", -1))
        return False
