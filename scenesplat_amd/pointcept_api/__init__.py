"""Host-side mirror of the pointcept interfaces the hot path sits behind (registries,
``Point``, ``PT-v3m1``, ``LangPretrainer`` + criteria, ``DefaultSegmentorV2`` + criteria, ``PDNorm`` / ``PPT-v1m2``, trainer/hook API, the training transforms, the open-vocabulary tester, the datasets and device loaders)."""
from .registry import HOOKS, LOSSES, MODELS, MODULES, PRETRAINERS, TESTERS, TRAINERS, TRANSFORMS, Registry, build_model  # noqa: F401
from .structure import Point  # noqa: F401
from . import ptv3  # noqa: F401  (registers PT-v3m1)
from . import lang  # noqa: F401  (registers LangPretrainer and the criteria)
from .ptv3 import PointTransformerV3, RUNTIME, bench_runtime  # noqa: F401
from .lang import LangPretrainer, build_criteria  # noqa: F401
from . import engine  # noqa: F401  (registers DefaultTrainer and the hooks)
from . import seg  # noqa: F401  (registers DefaultSegmentorV2, CrossEntropyLoss, LovaszLoss, SemSegEvaluator)
from .engine import HookBase, Trainer, TrainerBase, create_ddp_model  # noqa: F401
from . import transform  # noqa: F401  (registers the per-sample training transforms)
from .transform import Compose  # noqa: F401
from .transform import (CollectContrast, ContrastiveViewsGenerator_SSL, GSGaussianBlurVoxelOpc, RandomColorGrayScale,  # noqa: F401
                        RandomColorJitter, RandomColorSolarize, SphereCropRandomMaxPoints)   # (the self-supervised view generator)
from .transform import (Add, ContrastiveViewsGenerator, CropBoundary, HueSaturationTranslation, InstanceParser,  # noqa: F401
                        NormalizeCoord, PointClip, PositiveShift, RandomColorDrop, ShufflePoint)   # (the rest of the reference's transforms)
from . import ppt  # noqa: F401  (registers PPT-v1m2)
from .pdnorm import PDNorm  # noqa: F401  (registered in MODULES)
from . import tester  # noqa: F401  (registers ZeroShotSemSegTester)
from .tester import TesterBase, ZeroShotSemSegTester, final_metrics, gather_records, merge_records  # noqa: F401
from . import ssl  # noqa: F401  (registers PT-v3m1-simdino and DefaultContrastiverSimDinoV2; engine registers DefaultSSLPreTrainer)
from .ssl import (CosinePatchLoss, CosineScheduler, DefaultContrastiverSimDinoV2, DINOHead, MCRLoss,  # noqa: F401
                  PointTransformerV3_SIMDINO)
from .engine import DefaultSSLPreTrainer  # noqa: F401
from . import datasets  # noqa: F401  (registers the dataset classes in DATASETS)
from .datasets import (DATASETS, ConcatDataset, DefaultDataset, DeviceLoader, GenericGSDataset, HoliCityGSDataset,  # noqa: F401
                       KITTI360GSDataset, Matterport3D_160_GSDataset, Matterport3DGSDataset, ScanNet200GSDataset, ScanNetGSDataset,
                       ScanNetPPGSDataset, build_dataset, build_test_loader, build_train_loader, build_val_loader)


def __getattr__(name):
    """preprocessing (scene chunking: writes the chunked splits the datasets read), chunk_scene, chunk_split: imported on first use,
    so that `python -m scenesplat_amd.pointcept_api.preprocessing` finds the module not yet imported and runs it once."""
    if name in ("preprocessing", "chunk_scene", "chunk_split"):
        import importlib
        module = importlib.import_module(".preprocessing", __name__)
        return module if name == "preprocessing" else getattr(module, name)
    # gaussian_ply (3DGS .ply checkpoints -> scene folders), likewise for `python -m scenesplat_amd.pointcept_api.gaussian_ply`
    if name in ("gaussian_ply", "read_ply_header", "load_gaussian_ply", "transfer_labels", "preprocess_gs"):
        import importlib
        module = importlib.import_module(".gaussian_ply", __name__)
        return module if name == "gaussian_ply" else getattr(module, name)
    # pc_labels (the labelled point cloud of the original scene -> scene and chunk folders), likewise for its command line
    if name in ("pc_labels", "slice_point_cloud", "attach_point_cloud"):
        import importlib
        module = importlib.import_module(".pc_labels", __name__)
        return module if name == "pc_labels" else getattr(module, name)
    # scannet_mesh (a raw ScanNet scan, and a checkpoint beside it -> the labelled scene folders), likewise for its command line
    if name in ("scannet_mesh", "read_mesh_header", "load_ply_mesh", "mesh_vertex_normals", "scannet_label_tables", "group_tables",
                "preprocess_scannet", "preprocess_scannet_gs"):
        import importlib
        module = importlib.import_module(".scannet_mesh", __name__)
        return module if name == "scannet_mesh" else getattr(module, name)
    # scannetpp_mesh (a raw ScanNet++ scan, and a checkpoint beside it -> the labelled scene folders), likewise for its command line
    if name in ("scannetpp_mesh", "scannetpp_classes", "first_groups", "mesh_vertex_normals_o3d", "multilabels", "preprocess_scannetpp",
                "preprocess_scannetpp_gs"):
        import importlib
        module = importlib.import_module(".scannetpp_mesh", __name__)
        return module if name == "scannetpp_mesh" else getattr(module, name)
    # oriented_box (the minimal oriented bounding box of a scan and the Gaussians inside it: `prune_box=` of the three converters)
    if name in ("oriented_box", "OrientedBox", "minimal_oriented_box", "points_within_box"):
        import importlib
        module = importlib.import_module(".oriented_box", __name__)
        return module if name == "oriented_box" else getattr(module, name)
    # feature_pca (PCA colours of a feature matrix on the device: `save_pca=` of the tester), likewise for its command line
    if name in ("feature_pca", "pca_colors", "fit_pca"):
        import importlib
        module = importlib.import_module(".feature_pca", __name__)
        return module if name == "feature_pca" else getattr(module, name)
    # text_query (text queries on saved features: scores, exact selection, the selected Gaussians as a scene folder), and its command line
    if name in ("text_query", "query_scene", "load_text_queries", "extract_geometry", "highlight_colors"):
        import importlib
        module = importlib.import_module(".text_query", __name__)
        return module if name == "text_query" else getattr(module, name)
    # render (a scene folder as alpha-composited Gaussian splats: an image tensor and a PNG, no viewer), and its command line
    if name in ("render", "render_scene", "look_at_camera", "fit_camera", "orbit_cameras", "save_image", "Camera"):
        import importlib
        module = importlib.import_module(".render", __name__)
        return module if name == "render" else getattr(module, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
