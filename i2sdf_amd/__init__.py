"""i2sdf_amd -- MI355X-native volume-rendering core for I2-SDF (hand-written HIP kernels behind the reference's
`I2SDFNetwork` module contract).  See DESIGN.md / INTEGRATION.md."""
from .config import NetConfig, SamplerConfig, synthetic_conf, plumbing_conf  # noqa: F401


def __getattr__(name):
    # torch-dependent pieces are imported lazily so that `import i2sdf_amd` stays cheap
    if name in ("I2SDFNetwork", "ImplicitNetwork", "RenderingNetwork", "LaplaceDensity"):
        from . import network
        return getattr(network, name)
    if name == "I2SDFLoss":
        from .loss import I2SDFLoss
        return I2SDFLoss
    if name in ("RayBatcher", "RaySample"):
        from . import batcher
        return getattr(batcher, name)
    if name == "FusedAdam":
        from .optim import FusedAdam
        return FusedAdam
    if name in ("BubblePDF", "depth_unproject"):
        from . import bubble
        return getattr(bubble, name)
    if name in ("GridAxes", "uniform_axes", "aligned_axes", "pca_frame"):
        from . import grid
        return getattr(grid, name)
    if name in ("marching_cubes", "Mesh", "face_components", "largest_component", "sample_surface", "compact",
                "voxel_down_sample", "nearest_neighbors", "evaluate", "mesh_depth", "tsdf_fuse", "tsdf_integrate", "tsdf_extract",
                "TsdfVolume", "refuse", "score", "MeshBVH", "RayHits", "build_bvh", "ray_mesh_intersect", "occluded", "ClosestPoints",
                "MeshNormals", "closest_point", "pseudonormals", "signed_distance", "surface_scores", "WindingMoments", "winding_moments",
                "winding_number", "inside", "simplify_vertex_clustering", "clean", "topology", "SimplifyResult", "CleanResult",
                "MeshTopology"):
        from . import mesh
        return getattr(mesh, name)
    if name in ("psnr", "ssim", "image_stats", "image_metrics", "to_frames", "interpolate_poses", "pixel_grid", "linear_to_srgb"):
        from . import views
        return getattr(views, name)
    if name in ("RenderingLayer", "get_rendering_parameters", "shade_draws"):
        from . import shading
        return getattr(shading, name)
    if name in ("KMeans", "kmeans_pp_centroid", "DBSCAN", "dbscan_seeds"):
        from . import cluster
        return getattr(cluster, name)
    if name in ("SphereTracer", "MeshTracer", "TraceResult", "TraceResultF"):
        from . import trace
        return getattr(trace, name)
    if name == "RenderEngine":
        from .engine import RenderEngine
        return RenderEngine
    raise AttributeError(name)
