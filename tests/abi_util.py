"""What the host tests share when they call the C ABI with arguments it must refuse (no GPU needed).  Not a test module."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                                  # non-null, 16-byte aligned; never dereferenced


def refused(lib, rc, who=None):
    """The call was refused (nothing may launch); its message, which with `who` starts with that symbol's name."""
    assert rc != 0
    msg = lib.lrf_last_error().decode()
    if who is not None:
        assert msg.startswith(who + ": "), msg
    return msg


def declared_exported_bound(lib, symbols):
    """Every symbol is in _native.SYMBOLS, declared in include/lrf.h and exported by the library.  Returns the header's text."""
    from localrf_amd import _native as N
    header = open(os.path.join(ROOT, "include", "lrf.h")).read()
    for name in symbols:
        assert name in N.SYMBOLS and f"{name}(" in header, name
        getattr(lib, name)
    return header


def filled(struct_cls, defaults, **over):
    """A struct with the defaults, then the overrides, set; a tuple or list goes element-wise into an array member."""
    a = struct_cls()
    for values in (defaults, over):
        for k, v in values.items():
            if isinstance(v, (tuple, list)):
                for i, o in enumerate(v):
                    getattr(a, k)[i] = o
            else:
                setattr(a, k, v)
    return a
