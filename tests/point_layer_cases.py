"""The launch sequences of the point-side Python layer (cloud.py, mesh_distance.py, alignment.py): for each public call on the
small cases the GPU tests already use, the list of (symbol, that launch's count argument).  tests/golden/point_layer_launches.json
holds these lists as the code gave them before the layer's checks, device step and batcher were shared; the GPU test asserts
that they still come out the same: the same launches, in the same order, chunked the same way.  Public names only."""
import numpy as np

from align_cases import blob, move_poses, sim, sim_inverse, source_cloud, trajectory, truth
from cloud_cases import cases as cloud_cases
from cloud_cases import icp_case, surface_with_floaters
from cloud_normal_cases import cases as normal_cases
from localrf_amd import _native, alignment, cloud, mesh_distance
from mesh_distance_cases import cases as mesh_cases
from mesh_raster_cases import octa_sphere
from mesh_util import device_mesh, to_dev

# symbol -> where its count lies: the position among the arguments after the device, or the field of the struct passed first
COUNT_AT = {"lrf_cloud_index_bounds": 1, "lrf_cloud_index_build": "M", "lrf_cloud_closest": 2, "lrf_cloud_knn": 2, "lrf_cloud_radius_count": 2,
            "lrf_cloud_normals": 2, "lrf_cloud_voxel_bounds": 1, "lrf_cloud_voxel": "M", "lrf_distance_summary": 1, "lrf_mesh_index_bounds": 3,
            "lrf_mesh_index_build": "Nf", "lrf_mesh_closest": 2, "lrf_mesh_sample_count": 3, "lrf_mesh_sample_emit": 6, "lrf_align_transform": 2,
            "lrf_align_pairs": 4, "lrf_align_plane": "N", "lrf_align_plane_cloud": "N", "lrf_select": 4}


def count_of(name, args):
    at = COUNT_AT[name]
    return int(getattr(args[0]._obj, at) if isinstance(at, str) else args[at])


def launch_lists():
    """name of the call -> [[symbol, count], ...], on the current GPU."""
    log, real = [], _native.launch

    def recording(name, dev, *args, **kw):
        log.append([name, count_of(name, args)])
        return real(name, dev, *args, **kw)

    out = {}

    def run(label, fn):
        del log[:]
        result = fn()
        out[label] = [list(x) for x in log]
        return result

    _native.launch = recording
    try:
        c = cloud_cases()["triplicates on themselves"]
        pts = to_dev(c["cloud"])
        index = run("CloudIndex", lambda: cloud.CloudIndex(pts))
        run("CloudIndex.closest", lambda: index.closest(pts, c["max_distance"], closest=True))
        run("CloudIndex.knn", lambda: index.knn(pts, 3, c["max_distance"], exclude_self=True))
        run("CloudIndex.radius_count", lambda: index.radius_count(pts, c["radius"], exclude_self=True))
        run("CloudIndex.normals", lambda: index.normals(pts, 0.5, viewpoint=pts + 1.0))
        run("voxel_downsample", lambda: cloud.voxel_downsample(pts, 0.25))
        run("nearest_spacing", lambda: cloud.nearest_spacing(index))
        n = normal_cases()["random M=65"]
        for order in cloud.NORMAL_ORDERS:
            run(f"estimate_normals {order}", lambda: cloud.estimate_normals(to_dev(n["cloud"]), n["radius"], order=order))
        sheet, _, radius = surface_with_floaters()
        run("remove_outliers", lambda: cloud.remove_outliers(to_dev(sheet), radius, 6))
        other = to_dev(cloud_cases()["triplicates"]["queries"])
        run("cloud_to_cloud", lambda: cloud.cloud_to_cloud(other, pts, (0.1, 0.2), 0.5))
        run("cloud_distance voxel", lambda: cloud.cloud_distance(other, pts, (0.1,), voxel=0.25))

        m = mesh_cases()["octa 512 default cell"]
        mesh, q = device_mesh(m["mesh"], rgb=False), to_dev(m["points"])
        mi = run("MeshIndex", lambda: mesh_distance.MeshIndex(mesh))
        run("MeshIndex.closest", lambda: mi.closest(q, closest=True))
        run("cloud_to_mesh", lambda: mesh_distance.cloud_to_mesh(q, mesh, (0.1,), 0.5))
        run("mesh_distance", lambda: mesh_distance.mesh_distance(device_mesh(octa_sphere(2), rgb=False), mesh, 0.1, (0.05,)))

        A, B, _, _, _ = icp_case()
        src, tgt = to_dev(A), to_dev(B)
        run("fit_pairs", lambda: alignment.fit_pairs(src, tgt, scale=False))
        gt = trajectory()
        est = move_poses(gt, sim_inverse(sim(0.6, 1.15, 0.0, axis=(1.0, 0.5, -2.0), t=(0.1, -0.1, 0.05))))
        run("trajectory_error", lambda: alignment.trajectory_error(to_dev(est), to_dev(gt)))
        blob_cloud = to_dev(source_cloud(truth(0, True)))
        run("icp mesh plane", lambda: alignment.icp(blob_cloud, device_mesh(blob(), rgb=False), iterations=2))
        scan = cloud.CloudIndex(tgt)
        run("icp cloud point", lambda: alignment.icp(src, scan, metric="point", iterations=2, max_distance=0.5))
        normals = cloud.estimate_normals(scan, 0.2)["normals"]
        run("icp cloud plane", lambda: alignment.icp(src, scan, metric="plane", target_normals=normals, iterations=2))
    finally:
        _native.launch = real
    assert all(out.values()) and np.all([isinstance(n, int) for rows in out.values() for _, n in rows])
    return out
