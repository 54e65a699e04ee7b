"""What the mesh test files share, one definition each: host arrays and meshes on the device, exact comparisons of meshes, the
24^3 blob volumes, the stub volumes on the CPU, and the monkeypatches that forbid or record native calls and renders.  Where the
files' own copies had drifted apart, a helper here asserts everything that any copy asserted."""
import functools

import numpy as np
import torch

from localrf_amd import _native, mesh, novel_views
from mesh_cases import H_ANALYTIC
from mesh_clean_cases import blobs_field

DEV = "cuda:0"


def to_dev(a):
    """A host array as a contiguous tensor on the device, dtype kept."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_mesh(m, rgb=True, **extra):
    """A host mesh dict as a mesh dict on the device: counts from the shapes, rgb8 where the mesh has one and rgb is wanted;
    extra entries (such as note="kept") are carried along."""
    c = m.get("rgb8") if rgb else None
    return dict(vertices=to_dev(m["vertices"]), faces=to_dev(m["faces"]), rgb8=None if c is None else to_dev(c),
                counts=(int(m["vertices"].shape[0]), int(m["faces"].shape[0])), **extra)


def cpu_mesh(rgb=True):
    """Four vertices and two faces in CPU tensors: valid everywhere but for its device."""
    return {"vertices": torch.zeros(4, 3), "faces": torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32),
            "rgb8": torch.zeros(4, 3, dtype=torch.uint8) if rgb else None, "counts": (4, 2)}


def bits(a):
    """The uint32 words of an fp32 tensor or of an array (taken as fp32)."""
    if torch.is_tensor(a):
        assert a.dtype is torch.float32
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """Two device tensors, or two dicts of them, exact: keys, shapes, dtypes, integers, and fp32 as its 32-bit words."""
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            same_bits(a[k], b[k])
        return
    assert a.shape == b.shape and a.dtype is b.dtype
    assert torch.equal(a.view(torch.int32) if a.dtype is torch.float32 else a, b.view(torch.int32) if b.dtype is torch.float32 else b)


def same_mesh(got, want):
    """A device mesh against a host expectation: counts, shapes, dtypes, vertices (as uint32), faces and rgb8, all exact."""
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    nv, nf = want["counts"]
    assert tuple(got["vertices"].shape) == (nv, 3) and tuple(got["faces"].shape) == (nf, 3)
    assert got["vertices"].dtype is torch.float32 and got["faces"].dtype is torch.int32
    assert np.array_equal(bits(got["vertices"]), want["vertices"].view(np.uint32))
    assert np.array_equal(got["faces"].cpu().numpy(), want["faces"])
    if want["rgb8"] is None:
        assert got["rgb8"] is None
    else:
        assert got["rgb8"].dtype is torch.uint8 and tuple(got["rgb8"].shape) == (nv, 3)
        assert np.array_equal(got["rgb8"].cpu().numpy(), want["rgb8"])


def same_device_mesh(a, b):
    """Two device meshes, exact: counts, vertex bits, faces, rgb8, and normals, normal_info and smooth where either has them."""
    assert a["counts"] == b["counts"]
    assert torch.equal(a["vertices"].view(torch.int32), b["vertices"].view(torch.int32)) and torch.equal(a["faces"], b["faces"])
    assert (a["rgb8"] is None) == (b["rgb8"] is None) and (a["rgb8"] is None or torch.equal(a["rgb8"], b["rgb8"]))
    assert ("normals" in a) == ("normals" in b)
    if "normals" in a:
        assert torch.equal(a["normals"].view(torch.int32), b["normals"].view(torch.int32)) and a["normal_info"] == b["normal_info"]
    assert a.get("smooth") == b.get("smooth")


@functools.lru_cache(maxsize=None)
def blob_volumes(origin=(0.0, 0.0, 0.0)):
    """(dense with colours, sparse without) over mesh_clean_cases.blobs_field(): 24^3 points, every one of the 27 blocks
    stored, six closed shells of 2902 vertices and 5780 faces."""
    fld = blobs_field()
    rgb = np.random.default_rng(12).uniform(0.0, 1.0, fld.shape + (3,)).astype(np.float32)
    dense = mesh.TsdfVolume(origin, H_ANALYTIC, (24, 24, 24), 3 * H_ANALYTIC, DEV)
    dense.tsdf.copy_(to_dev(fld))
    dense.weight.fill_(1.0)
    dense.rgb.copy_(to_dev(rgb))
    sparse = mesh.SparseTsdfVolume(origin, H_ANALYTIC, (3, 3, 3), 3 * H_ANALYTIC, DEV, colours=False)
    sparse.marks.fill_(1)
    assert sparse.allocate() == 27
    sparse.tsdf.copy_(to_dev(np.ascontiguousarray(fld.reshape(3, 8, 3, 8, 3, 8).transpose(0, 2, 4, 1, 3, 5).reshape(27, 8, 8, 8))))
    sparse.weight.fill_(1.0)
    return dense, sparse


class DenseStub(mesh.TsdfVolume):
    """A TsdfVolume on the CPU, for the refusals that come before the device check."""
    def __init__(self, colours=True):
        self.origin, self.voxel, self.dims, self.trunc = (0.0, 0.0, 0.0), 0.1, (3, 3, 3), 0.3
        self.tsdf, self.weight = torch.ones(3, 3, 3), torch.zeros(3, 3, 3)
        self.rgb = torch.zeros(3, 3, 3, 3) if colours else None


class SparseStub(mesh.SparseTsdfVolume):
    """A SparseTsdfVolume without blocks on the CPU, for the refusals that come before the device check."""
    def __init__(self, colours=True):
        self.origin, self.voxel, self.blocks, self.dims, self.trunc, self.colours = (0.0, 0.0, 0.0), 0.1, (2, 2, 2), (16, 16, 16), 0.3, colours
        self.marks, self.table, self.n_blocks = torch.zeros(2, 2, 2, dtype=torch.uint8), torch.full((2, 2, 2), -1, dtype=torch.int32), 0
        self._coords = torch.zeros(1, 3, dtype=torch.int32)
        self._tsdf, self._weight = torch.ones(0, 8, 8, 8), torch.zeros(0, 8, 8, 8)
        self._rgb = torch.zeros(0, 8, 8, 8, 3) if colours else None


def forbid_native(monkeypatch):
    """No native call is reached from here on: neither a launch, nor a plain call, a workspace or the library itself."""
    def forbidden(*a, **k):
        raise AssertionError("a native call was reached")
    for name in ("launch", "call", "workspace", "lib"):
        monkeypatch.setattr(_native, name, forbidden)


def forbid_render(monkeypatch, *also):
    """No render is reached from here on: novel_views.render_poses, and every (module, name) of `also`, raises."""
    def forbidden(*a, **k):
        raise AssertionError("a render was reached before the refusal")
    for module, name in ((novel_views, "render_poses"),) + also:
        monkeypatch.setattr(module, name, forbidden)


def record_launches(monkeypatch):
    """-> the list that the symbol name of every _native.launch from here on is appended to; the launches go through."""
    names, real = [], _native.launch

    def recording(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(_native, "launch", recording)
    return names
