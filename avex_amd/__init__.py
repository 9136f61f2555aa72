"""avex_amd — MI355X-native embedding-extraction path behind the AVEX plugin API.

Public surface mirrors ``import avex`` (reference: avex/__init__.py:11-51) for the hot path:
``load_model`` -> model with ``forward`` / ``extract_embeddings`` / ``register_hooks_for_layers``.
The arithmetic lives in ``avex_amd/lib/libavexhip.so`` (hand-written HIP for gfx950, C ABI in
``include/avexhip.h``); importing this package does not need a GPU, running a model does.
"""
from .configs import AudioConfig, ModelSpec
from .load import build_model, build_model_from_spec, load_label_mapping, load_model
from .registry import (describe_model, get_checkpoint_path, get_model_class, get_model_spec, list_model_classes,
                       list_model_layers, list_models, register_model, register_model_class)
from .base_model import ModelBase
from .search import EmbeddingIndex, query_by_example
from .detection import decode_events, detect_events
from .examples import ExampleBank, detect_events_by_example
from .density import dbscan, k_distance
from .activity import ActivityGate, band_activity
from .annotations import Annotations, score_events, sweep_thresholds
from .soundscape import IndexSpec, acoustic_indices, spectral_stats
from .measurements import MeasureSpec, measure_boxes, measure_events, noise_spectrum, write_raven
from .regions import RegionSpec, find_regions, label_cells

__version__ = "0.1.0"

__all__ = [
    "load_model", "register_model", "get_model_spec", "list_models", "describe_model", "list_model_layers",
    "register_model_class", "get_model_class", "list_model_classes", "build_model", "build_model_from_spec",
    "get_checkpoint_path", "load_label_mapping", "ModelBase", "ModelSpec", "AudioConfig", "EmbeddingIndex", "query_by_example",
    "decode_events", "detect_events", "ExampleBank", "detect_events_by_example", "dbscan", "k_distance",
    "ActivityGate", "band_activity", "Annotations", "score_events", "sweep_thresholds",
    "IndexSpec", "acoustic_indices", "spectral_stats",
    "MeasureSpec", "measure_boxes", "measure_events", "noise_spectrum", "write_raven",
    "RegionSpec", "find_regions", "label_cells",
]
