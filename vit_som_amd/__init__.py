"""vit_som_amd: MI355X-native (gfx950) ViT-SOM training step behind the reference's
``ViTSOM`` / ``SOMLayer`` module surface (models/vit_som.py, models/som_layer.py).

Layers, lowest first: ``_lib`` / ``ops`` (the C-ABI), ``arena``, ``tuning`` and ``_base``; ``vit``
(ViTAutoencoder) and ``som`` (SOMLayer); ``optim`` (FusedAdamW) and ``step`` (the fused step's
machinery shared by every arena-owning model); ``vit_owner`` (what the two ViT models share);
``model`` (ViTSOM), ``classifier`` (ViTClassifier, the plain ViT baseline) and ``desom`` (DESOM),
three peers; ``plots`` (host-only drawing) under ``evaluation``."""
from . import _lib  # noqa: F401  (fails loudly when libvitsom_hip.so is absent)
from . import ops  # noqa: F401
from .vit import ViTAutoencoder  # noqa: F401,E402
from .som import BatchSOMReport, SOMLayer  # noqa: F401,E402
from .optim import FusedAdamW, param_groups_lrd  # noqa: F401,E402
from .model import ViTSOM  # noqa: F401,E402
from .desom import DESOM, Autoencoder  # noqa: F401,E402
from .classifier import ViTClassifier  # noqa: F401,E402
from . import evaluation  # noqa: F401,E402
from .evaluation import KNNReport, MapQuality, evaluate_knn, evaluate_map_quality, visualize_umap_map  # noqa: F401,E402
from .evaluation import EmbeddingQualityReport, MapNeighbourhood, evaluate_embedding_quality, map_neighbourhood  # noqa: F401,E402
from .embedding_quality import EmbeddingQuality, continuity, embedding_quality, rank_penalties, trustworthiness  # noqa: F401,E402
from .silhouette import SilhouetteReport, cluster_silhouette, silhouette_samples, silhouette_score  # noqa: F401,E402
from .evaluation import evaluate_silhouette, visualize_silhouette_map  # noqa: F401,E402
from .pca import PCA  # noqa: F401,E402
from .evaluation import LatentSpectrum, evaluate_latent_spectrum, init_som_from_data, visualize_pca_map  # noqa: F401,E402
from .evaluation import fit_som_batch  # noqa: F401,E402
from .kmeans import KMeans, kmeans_plusplus  # noqa: F401,E402
from .umap import UMAP  # noqa: F401,E402
from .knn import KNNClassifier  # noqa: F401,E402
from .linear_probe import LinearProbeReport, LogisticRegression, evaluate_linear_probe  # noqa: F401,E402
from .gmm import GaussianMixture, GMMReport, evaluate_gmm  # noqa: F401,E402
from .agglomerative import AgglomerativeClustering, MapClustersReport, evaluate_map_clusters, visualize_map_clusters  # noqa: F401,E402
from .dbscan import DBSCAN, DBSCANReport, evaluate_dbscan, k_distances, visualize_dbscan  # noqa: F401,E402
from .hdbscan import HDBSCAN, HDBSCANReport, evaluate_hdbscan, visualize_hdbscan  # noqa: F401,E402
from .spectral import SpectralClustering, SpectralEmbedding, SpectralReport, evaluate_spectral, visualize_spectral_map  # noqa: F401,E402
from .attention_rollout import AttentionReport, evaluate_attention, visualize_attention_map, visualize_attention_rollout  # noqa: F401,E402
from .tsne import TSNE, TSNEQualityReport, evaluate_tsne_quality, visualize_tsne_progression  # noqa: F401,E402
from .data import DeviceDataset, DeviceLoader, DeviceTransform  # noqa: F401,E402
