"""The public surface of vit_som_amd.evaluation, pinned: the signature of every public callable (and of the two private
helpers other tests import), the fields of its dataclasses, and the identity of what the package re-exports.  The table
was printed from the module as it stood before its scaffolding was folded into one adapter and one loader pass."""
import dataclasses
import inspect

SIGNATURES = {
    'EmbeddingQualityReport': '(trustworthiness: float, continuity: float, n_neighbors: int, n_samples: int, trust_penalty: int, cont_penalty: int, trust_per_row: numpy.ndarray, cont_per_row: numpy.ndarray, embedding: numpy.ndarray = None, fitted_rows: numpy.ndarray = None, fitted: tuple = None, transformed: tuple = None, inference_time: float = 0.0) -> None',
    'KNNReport': '(accuracy: float, per_class_accuracy: numpy.ndarray, confusion: numpy.ndarray, n_train: int, n_test: int, k: int, inference_time: float) -> None',
    'LatentSpectrum': '(explained_variance: numpy.ndarray, explained_variance_ratio: numpy.ndarray, cumulative_ratio: numpy.ndarray, total_variance: float, components_for: dict, effective_rank: float, residuals: numpy.ndarray, n_samples: int, inference_time: float = 0.0) -> None',
    'MapNeighbourhood': '(neighbours: numpy.ndarray, ranks: numpy.ndarray, mean_rank: float, within_degree: float) -> None',
    'MapQuality': '(quantization_error: float, topographic_error: float, hits: numpy.ndarray, dead_units: int, cell_quantization_error: numpy.ndarray, nearest_sample: numpy.ndarray, nearest_distance: numpy.ndarray, n_samples: int, inference_time: float) -> None',
    '_key_to_float': '(key)',
    '_som_latents': '(model, config, dataloader, who)',
    'calculate_purity': '(y_trues, y_preds)',
    'classification_from_table': '(cm: numpy.ndarray)',
    'components_for': '(cumulative_ratio, shares=(0.5, 0.9, 0.95, 0.99))',
    'decode_prototype': '(vit, prototype, num_patches, embed_dim, device)',
    'decoded_prototype_canvas': '(model, config, chunk=512, gap=1)',
    'draw_decoded_prototypes': '(canvas, output_dir, model_arch, epoch)',
    'draw_label_heatmap': '(heatmap, output_dir, model_arch, epoch)',
    'effective_rank': '(eigenvalues) -> float',
    'evaluate_classification': '(model, config, dataloader)',
    'evaluate_clustering': '(model, config, dataloader, num_labels=None)',
    'evaluate_embedding_quality': '(model, config, dataloader, n_neighbors=15, fit_rows=None)',
    'evaluate_kmeans': '(model, config, dataloader, num_labels=None)',
    'evaluate_knn': "(model, config, train_loader, test_loader, k=20, weights='softmax', metric='cosine', temperature=0.07, bank_rows=4096, num_labels=None)",
    'evaluate_latent_spectrum': '(model, config, dataloader, n_components=64)',
    'evaluate_map_quality': '(model, config, dataloader)',
    'evaluate_silhouette': "(model, config, dataloader, clusters='bmu', metric=None, n_clusters=None, sample_size=None)",
    'fit_som_batch': '(model, config, dataloader, epochs=10, init=None, sigma=None, max_rows=None)',
    'init_som_from_data': "(model, config, dataloader, method='pca', max_rows=None)",
    'map_neighbourhood': '(model)',
    'nmi_from_table': '(w: numpy.ndarray) -> float',
    'purity_from_table': '(w: numpy.ndarray) -> float',
    'umatrix': '(model)',
    'visualize_decoded_prototypes': "(model, config, output_dir='experiments/plots', return_decoded=False, chunk=512, gap=1)",
    'visualize_hit_map': "(model, config, dataloader, output_dir='experiments/plots')",
    'visualize_label_heatmap': "(model, config, dataloader, output_dir='experiments/plots')",
    'visualize_pca_map': "(model, config, dataloader, epoch=0, output_dir='experiments/plots/vit_som/pca')",
    'visualize_silhouette_map': "(model, config, dataloader, output_dir='experiments/plots', metric=None)",
    'visualize_umap_map': "(model, config, dataloader, epoch=0, output_dir='experiments/plots/vit_som/umap', fit_rows=None)",
    'visualize_umap_progression': "(model, config, dataloader, epoch=0, output_dir='experiments/plots/vit_som/umap', fit_rows=None)",
    'visualize_umatrix': "(model, config, output_dir='experiments/plots')",
}

FIELDS = {
    'EmbeddingQualityReport': ['trustworthiness', 'continuity', 'n_neighbors', 'n_samples', 'trust_penalty', 'cont_penalty', 'trust_per_row', 'cont_per_row', 'embedding', 'fitted_rows', 'fitted', 'transformed', 'inference_time'],
    'KNNReport': ['accuracy', 'per_class_accuracy', 'confusion', 'n_train', 'n_test', 'k', 'inference_time'],
    'LatentSpectrum': ['explained_variance', 'explained_variance_ratio', 'cumulative_ratio', 'total_variance', 'components_for', 'effective_rank', 'residuals', 'n_samples', 'inference_time'],
    'MapNeighbourhood': ['neighbours', 'ranks', 'mean_rank', 'within_degree'],
    'MapQuality': ['quantization_error', 'topographic_error', 'hits', 'dead_units', 'cell_quantization_error', 'nearest_sample', 'nearest_distance', 'n_samples', 'inference_time'],
}

REEXPORTED = ['EmbeddingQualityReport', 'KNNReport', 'LatentSpectrum', 'MapNeighbourhood', 'MapQuality', 'evaluate_embedding_quality',
              'evaluate_knn', 'evaluate_latent_spectrum', 'evaluate_map_quality', 'evaluate_silhouette', 'fit_som_batch',
              'init_som_from_data', 'map_neighbourhood', 'visualize_pca_map', 'visualize_silhouette_map', 'visualize_umap_map']

OWN_MODULES = ("vit_som_amd.evaluation", "vit_som_amd.plots")     # the drawing helpers live in plots and are imported back


def test_signatures_are_those_of_the_table():
    from vit_som_amd import evaluation
    got = {name: str(inspect.signature(getattr(evaluation, name))) for name in SIGNATURES}
    assert got == SIGNATURES


def test_no_public_callable_came_or_went():
    from vit_som_amd import evaluation
    public = {name for name, obj in vars(evaluation).items()
              if not name.startswith("_") and callable(obj) and getattr(obj, "__module__", None) in OWN_MODULES}
    assert public == {name for name in SIGNATURES if not name.startswith("_")}


def test_dataclass_fields_are_those_of_the_table():
    from vit_som_amd import evaluation
    classes = {name for name, obj in vars(evaluation).items()
               if dataclasses.is_dataclass(obj) and obj.__module__ == "vit_som_amd.evaluation"}
    assert classes == set(FIELDS)
    assert {name: [f.name for f in dataclasses.fields(getattr(evaluation, name))] for name in FIELDS} == FIELDS


def test_the_package_reexports_the_same_objects():
    import vit_som_amd
    from vit_som_amd import evaluation
    for name in REEXPORTED:
        assert getattr(vit_som_amd, name) is getattr(evaluation, name), name
    # and nothing the package takes from evaluation is missing from the list
    taken = {name for name, obj in vars(vit_som_amd).items()
             if getattr(obj, "__module__", None) == "vit_som_amd.evaluation" and not name.startswith("_")}
    assert taken == set(REEXPORTED)
