"""localrf_amd -- MI355X-native render path of facebookresearch/localrf.

Public surface mirrors the reference's names:
  TensorVMSplit, AlphaGridMask      (models/tensoRF.py, models/tensorBase.py)
  LocalTensorfs                     (local_tensorfs.py)
  rays.*                            (utils/ray_utils.py, utils/utils.py 6D helpers)
  FusedAdam                         (torch.optim.Adam as local_tensorfs.py:88-97,146 configures it)
  losses.flow_loss / depth_loss     (train.py:385-423 with utils/utils.py:15-59)
  metrics.rgb_ssim / test_view_metrics (utils/utils.py:232-287, renderer.py:155-167: test-view SSIM and MSE)
  diagnostics.quantile / median / flow_comparison / depth_comparison / test_view_evaluation
                                    (renderer.py:79-124: test-view flow and depth comparison images, exact device quantiles)
  DeviceFrames                      (dataLoader/localrf_dataset.py, train split: a device-resident frame window)
  novel_views.render_poses / iter_pose_frames / encode_frames / visualize_depth / nearest_frames
                                    (renderer.py:43-77,130-148, test=False: novel camera poses, frames encoded on the device)
  pointcloud.backproject / fuse_points / scene_point_cloud / write_ply
                                    (rendered depth fused into a filtered, coloured world-space point cloud; no reference row)
  normals.render_normals / encode_normals, TensorVMSplit.render_normals / density_gradient
                                    (per-ray surface normals from the density gradient: normal maps, PLY normals; no reference row)
  depth_quantiles.render_depth_quantiles / median_depth, TensorVMSplit.render_depth_quantiles
                                    (median and quantile ray depth: the depth a fusion wants; no reference row)
  mesh.TsdfVolume / extract_mesh / scene_mesh
                                    (rendered depth fused into a TSDF volume, marching tetrahedra, PLY faces; no reference row)
  mesh.SparseTsdfVolume / scene_mesh(sparse=True)
                                    (the same volume stored in 8 x 8 x 8 blocks where depth reaches: long scenes; no reference row)
  mesh_raster.rasterize / depth_agreement / scene_mesh_agreement
                                    (a mesh rasterised back into camera poses and compared with rendered depth; no reference row)
  mesh_texture.TextureBaker / scene_texture / face_uv / sample_texture / write_obj
                                    (a texture atlas baked for a mesh from rendered frames, OBJ + PNG export; no reference row)
  mesh_distance.MeshIndex / sample_surface / distance_summary / cloud_to_mesh / mesh_distance
                                    (point-to-mesh distance: surface error, Chamfer, Hausdorff and F-score; no reference row)
  cloud.CloudIndex / voxel_downsample / nearest_spacing / remove_outliers / cloud_to_cloud / cloud_distance
                                    (a neighbour index over a point cloud: nearest, k nearest and radius queries, voxel grid,
                                    outlier removal, cloud-to-cloud Chamfer and F-score against a scan; no reference row)
  cloud.estimate_normals / CloudIndex.normals
                                    (normals, eigenvalues and surface variation of a bare point cloud by PCA over radius
                                    neighbourhoods; point-to-plane alignment.icp against a scan takes them; no reference row)
  alignment.fit_pairs / trajectory_error / icp / align_meshes / transform_points / transform_mesh
                                    (similarity registration of trajectories, clouds and meshes: closed-form fit from exact
                                    integer moments, point-to-plane ICP, trajectory error after alignment; no reference row)
The arithmetic of TensorVMSplit.forward and of LocalTensorfs.forward (ray generation, field
blend, exposure) runs in hand-written HIP kernels for gfx950 (csrc/), reached through the C ABI
of include/lrf.h.
"""
from ._native import NativeError  # noqa: F401
from .field import TensorVMSplit, AlphaGridMask, MLPRender_Fea_late_view  # noqa: F401
from .scene import LocalTensorfs  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from . import rays  # noqa: F401
from . import losses  # noqa: F401
from . import metrics  # noqa: F401
from . import diagnostics  # noqa: F401
from . import novel_views  # noqa: F401
from . import pointcloud  # noqa: F401
from . import normals  # noqa: F401
from . import depth_quantiles  # noqa: F401
from . import mesh  # noqa: F401
from . import mesh_raster  # noqa: F401
from . import mesh_texture  # noqa: F401
from . import mesh_distance  # noqa: F401
from . import cloud  # noqa: F401
from . import alignment  # noqa: F401
from .frames import DeviceFrames  # noqa: F401

__all__ = ["TensorVMSplit", "AlphaGridMask", "MLPRender_Fea_late_view", "LocalTensorfs", "rays", "losses", "metrics", "diagnostics", "novel_views", "pointcloud", "normals", "depth_quantiles", "mesh", "mesh_raster", "mesh_texture", "mesh_distance", "cloud", "alignment", "NativeError", "FusedAdam", "DeviceFrames"]
