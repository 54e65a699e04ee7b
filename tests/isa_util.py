"""What the host tests share when they read the gfx950 assembly of the library (no GPU needed): the one compile, as
__graft_entry__.build() compiles it, and the readers of a kernel's body and metadata.  Not a test module."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "localrf_amd", "csrc", "lrf_render.hip")
BUILD_FLAGS = ["-fno-slp-vectorize"]            # = __graft_entry__.build()


def device_asm(extra=BUILD_FLAGS):
    """The device assembly of the whole library; compiled once per process and set of flags."""
    return _device_asm(tuple(extra))


@functools.lru_cache(maxsize=None)
def _device_asm(extra):
    import __graft_entry__ as ge
    src = open(ge.__file__).read()
    assert all(f in src for f in BUILD_FLAGS), "the tests must compile with the flags of __graft_entry__.build()"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17"] + list(extra) + ["-I",
                               os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", out, SRC],
                              stderr=subprocess.DEVNULL)
        return open(out).read()


@functools.lru_cache(maxsize=2)
def kernels(asm):
    """name -> body text of every kernel in the assembly."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel", asm, re.S | re.M):
        out[m[1]] = m[2]
    return out


def find(asm, pattern):
    """The (mangled name, body) pairs whose name matches; at least one."""
    hits = [(k, v) for k, v in kernels(asm).items() if re.search(pattern, k)]
    assert hits, pattern
    return hits


def meta(asm, mangled):
    """The text of the kernel's .amdhsa_kernel ... .end_amdhsa_kernel block."""
    text = asm[asm.index(".amdhsa_kernel " + mangled):]
    return text[:text.index(".end_amdhsa_kernel")]


def scratch_bytes(asm, mangled):
    priv = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta(asm, mangled))
    assert priv, mangled
    return int(priv[1])


def vgprs(asm, mangled):
    """From the kernel-info comment, which follows the metadata block in the text behind the kernel's label."""
    text = asm[asm.index(mangled + ":"):]
    vg = re.search(r"; NumVgprs: (\d+)", text[:text.index(".end_amdhsa_kernel") + 4000])
    assert vg, mangled
    return int(vg[1])


def assert_no_scratch(asm, names, match, total=None, body_too=False):
    """No kernel of `names` has a private segment.  match = "exact": the function of that name, one hit each; "prefix": the name
    may go on (a template instance), one hit each; "search": find() per name, `total` hits in all.  With body_too no body
    holds a scratch instruction either.  Returns the (mangled name, body) pairs in the order found."""
    if match == "search":
        found = [hit for name in names for hit in find(asm, name)]
        assert len(found) == total, (total, [n for n, _ in found])
    else:
        tail = {"exact": r"E\w*)", "prefix": r"\w*)"}[match]
        found = []
        for name in names:
            hits = re.findall(r"\.amdhsa_kernel (_Z\w*?\d+" + name + tail, asm)
            assert len(hits) == 1, (name, hits)
            found.append((hits[0], kernels(asm)[hits[0]]))
    for mangled, body in found:
        assert scratch_bytes(asm, mangled) == 0, (mangled, scratch_bytes(asm, mangled))
        if body_too:
            assert "scratch_" not in body, mangled
    return found
