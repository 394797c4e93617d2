"""Training driver equivalent to the reference's experiments/benchmarking/train_vit_som.py:27-130
 without Lightning: n_runs independent runs, seed 0, per-epoch LambdaLR stepping,
validation loop + best-by-val/accuracy checkpoint in classification mode, last-epoch checkpoint in
clustering mode, final evaluation (classification metrics on the test loader / purity + NMI of the
reloaded last checkpoint on the train loader), mean (std) report.

Data comes from a `make_loaders(config, rank, world_size)` callable returning
(train_loader, val_loader, test_loader); the reference's data/data.py:get_dataloaders needs
torchvision/timm and downloads (absent offline), so the default is a synthetic, class-structured
in-memory set of the configured shape; `device_loaders` (--device-data, --data-npz PATH) keeps the
images on the GPU as uint8 and applies the configs' crop / flip / erase augmentation there
(vit_som_amd.data); --device-randaug adds the configs' RandAugment and timm rand-m9 auto-augment.  One process per GPU: under torchrun (WORLD_SIZE > 1) every rank takes an
interleaved shard of each loader and gradients are summed by one RCCL all-reduce.

    python -m vit_som_amd.train --config configs/vit_som/vit_som_cifar-10.yaml [--runs 5] [--epochs N]

A config with hyperparameters.model_arch == "vit" (the reference's configs/vit/*.yaml) trains the ViT baseline,
ViTClassifier, as experiments/benchmarking/train_vit.py does.
"""
import argparse
import copy
import os
import shutil
import time

import numpy as np
import torch
import yaml

from .evaluation import (evaluate_classification, evaluate_clustering, evaluate_embedding_quality, evaluate_knn, evaluate_linear_probe,
                         evaluate_map_quality, evaluate_silhouette, evaluate_latent_spectrum, fit_som_batch,
                         evaluate_gmm, evaluate_map_clusters, evaluate_tsne_quality, init_som_from_data, evaluate_dbscan, evaluate_spectral,
                         evaluate_hdbscan)
from .attention_rollout import visualize_attention_map, visualize_attention_rollout
from .classifier import ViTClassifier
from .model import ViTSOM


def load_config(config_path="./configs/config.yaml"):
    """The YAML config as a nested dict; a non-empty DATASET_NAME in the environment replaces data.dataset
    (behaviour of tools/utils.py:14-26)."""
    with open(config_path) as fh:
        cfg = yaml.safe_load(fh)
    cfg["data"]["dataset"] = os.environ.get("DATASET_NAME") or cfg["data"]["dataset"]
    return cfg


def clear_directory(directory):
    """Start every run from an empty checkpoint directory (behaviour of train_vit_som.py:19-25)."""
    shutil.rmtree(directory, ignore_errors=True)
    os.makedirs(directory, exist_ok=True)


def _report(all_metrics, n_runs, dataset_name, log):
    """Mean (std) over the runs, in the reference's output format (train_vit_som.py:118-130)."""
    log(f"\n--- Aggregated Results Across {n_runs} Runs for {dataset_name} ---")
    timed = {"run_duration", "inference_time"}
    for key, scores in all_metrics.items():
        if not scores:
            continue
        mean, std = float(np.mean(scores)), float(np.std(scores))
        label = key.capitalize()
        log(f"Avg {label} (Std): {mean:.2f}s ({std:.2f}s)" if key in timed else f"{label} Mean (Std): {mean:.4f} ({std:.4f})")


class TensorLoader:
    """Minimal DataLoader stand-in over in-memory tensors: fixed batch size, optional per-epoch
    shuffle, rank-interleaved sharding; exposes .dataset with __len__ (som_layer.py:131)."""

    def __init__(self, x, y, batch_size, shuffle=False, rank=0, world_size=1, seed=0, drop_last=False):
        self.x, self.y, self.batch_size, self.shuffle = x, y, int(batch_size), shuffle
        self.rank, self.world, self.seed, self.drop_last, self.epoch = rank, world_size, seed, drop_last, 0
        self.dataset = torch.utils.data.TensorDataset(x, y)

    def __len__(self):
        n = len(self.dataset) // self.world
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        n = len(self.dataset)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + self.epoch)) if self.shuffle else torch.arange(n)
        self.epoch += 1
        idx = idx[: (n // self.world) * self.world][self.rank::self.world]
        for i in range(0, len(idx), self.batch_size):
            j = idx[i:i + self.batch_size]
            if self.drop_last and len(j) < self.batch_size:
                break
            yield self.x[j], self.y[j]


def synthetic_loaders(config, rank=0, world_size=1, n_train=2048, n_val=256, n_test=256, seed=0):
    """Class-structured synthetic images of the configured shape (each class = a fixed random
    template + noise), so that accuracy / purity move during training."""
    hp, d = config["hyperparameters"], config["data"]
    C, S = d["num_channels"], d["input_size"]
    ncls = max(int(d["num_classes"]), 1) if d["num_classes"] > 0 else 10
    g = torch.Generator().manual_seed(seed)
    templates = torch.randn(ncls, C, S, S, generator=g)

    def make(n):
        y = torch.randint(0, ncls, (n,), generator=g)
        return templates[y] + 0.5 * torch.randn(n, C, S, S, generator=g), y
    bs = hp["batch_size"]
    (xt, yt), (xv, yv), (xs, ys) = make(n_train), make(n_val), make(n_test)
    return (TensorLoader(xt, yt, bs, shuffle=True, rank=rank, world_size=world_size, seed=seed, drop_last=True),
            TensorLoader(xv, yv, bs, rank=rank, world_size=world_size), TensorLoader(xs, ys, bs, rank=rank, world_size=world_size))


def device_loaders(config, rank=0, world_size=1, n_train=2048, n_val=256, n_test=256, seed=0, npz=None, strict=False,
                   auto_augment=False):
    """A `make_loaders` whose input side runs on the device (vit_som_amd.data): the images live on the GPU as uint8, the train
    loader applies the config's training transform (crops, flip, random erasing), val / test the evaluation transform.
    Default data: synthetic_loaders' class-structured set, quantised to 8 bits (level = 255 clip(x / 4 + 1 / 2, 0, 1)).
    `npz`: a local file with `images` / `labels` (and optionally `test_images` / `test_labels`; without them the last tenth
    of the rows is held out) -- validation and test then share the held-out part.  `auto_augment`: the train loader also
    applies the config's RandAugment and timm rand-m9 auto-augment (DeviceTransform.from_config(auto_augment=True)).
    Images of different sizes: a file with an `offsets` key is a ragged set as tools/pack_images.py writes it (`data`,
    `offsets`, `shapes`, `labels`, `channels`, optionally the same under `test_`; otherwise the last tenth is held out), and
    a config that names a variable-size image set (flowers-17 / -102) without a file gets a synthetic ragged set of the
    same class structure with sides drawn in [S, 2 S].  Both go through RaggedDeviceDataset and the variable-size transform."""
    from .data import VARIABLE_SIZE_SETS, DeviceDataset, DeviceLoader, DeviceTransform, RaggedDeviceDataset
    hp, d = config["hyperparameters"], config["data"]
    C, S, bs = d["num_channels"], d["input_size"], hp["batch_size"]
    dev = torch.device("cuda", torch.cuda.current_device())
    ragged = False
    if npz is not None:
        with np.load(npz) as z:
            ragged = "offsets" in z
    if ragged:
        full = RaggedDeviceDataset.from_npz(npz, "cpu")
        with np.load(npz) as z:
            has_test = "test_offsets" in z
        if has_test:
            train_set = RaggedDeviceDataset.from_npz(npz, dev)
            val_set = test_set = RaggedDeviceDataset.from_npz(npz, dev, prefix="test_")
        else:
            k = len(full) - max(len(full) // 10, 1)
            cut = int(full.offsets[k])                         # image k starts the held-out part
            train_set = RaggedDeviceDataset(full.data[:cut], full.offsets[:k], full.shapes[:k], full.labels[:k], full.C, dev)
            val_set = test_set = RaggedDeviceDataset(full.data[cut:], full.offsets[k:] - cut, full.shapes[k:], full.labels[k:],
                                                     full.C, dev)
    elif npz is None and d["dataset"] in VARIABLE_SIZE_SETS and d["dataset"] != "reuters":
        ragged = True
        ncls = max(int(d["num_classes"]), 1) if d["num_classes"] > 0 else 10
        g = torch.Generator().manual_seed(seed)
        templates = (torch.randn(ncls, C, S, S, generator=g) / 4 + 0.5).clamp_(0, 1).mul_(255)

        def make(n):
            # a class = its template stretched to the image's own h x w (nearest pixel) plus noise of +-32 levels
            y = torch.randint(0, ncls, (n,), generator=g)
            sides = torch.randint(S, 2 * S + 1, (n, 2), generator=g)
            images = []
            for c, (h, w) in zip(y.tolist(), sides.tolist()):
                rows, cols = torch.arange(h) * S // h, torch.arange(w) * S // w
                img = templates[c][:, rows][:, :, cols] + torch.randint(-32, 33, (C, h, w), generator=g)
                images.append(img.clamp_(0, 255).to(torch.uint8).numpy())
            return RaggedDeviceDataset.from_arrays(images, y, dev, layout="CHW")
        train_set, val_set, test_set = make(n_train), make(n_val), make(n_test)
    elif npz is not None:
        with np.load(npz) as z:
            xi, yi = torch.from_numpy(z["images"]), torch.from_numpy(z["labels"].astype(np.int64))
            if "test_images" in z:
                xh, yh = torch.from_numpy(z["test_images"]), torch.from_numpy(z["test_labels"].astype(np.int64))
            else:
                k = len(xi) - max(len(xi) // 10, 1)
                (xi, xh), (yi, yh) = (xi[:k], xi[k:]), (yi[:k], yi[k:])
        train_set = DeviceDataset(xi, yi, dev)
        val_set = test_set = DeviceDataset(xh, yh, dev)
    else:
        ncls = max(int(d["num_classes"]), 1) if d["num_classes"] > 0 else 10
        g = torch.Generator().manual_seed(seed)
        templates = torch.randn(ncls, C, S, S, generator=g)

        def make(n):
            y = torch.randint(0, ncls, (n,), generator=g)
            x = templates[y] + 0.5 * torch.randn(n, C, S, S, generator=g)
            return DeviceDataset((x / 4 + 0.5).clamp_(0, 1).mul_(255).round_().to(torch.uint8), y, dev)
        train_set, val_set, test_set = make(n_train), make(n_val), make(n_test)
    t_train = DeviceTransform.from_config(config, True, strict=strict, auto_augment=auto_augment, variable_size=ragged)
    t_eval = DeviceTransform.from_config(config, False, variable_size=ragged)
    return (DeviceLoader(train_set, bs, t_train, shuffle=True, rank=rank, world_size=world_size, seed=seed, drop_last=True),
            DeviceLoader(val_set, bs, t_eval, rank=rank, world_size=world_size),
            DeviceLoader(test_set, bs, t_eval, rank=rank, world_size=world_size))


def fit(model, config, train_loader, val_loader, ckpt_dir, dataset_name, use_validation, max_epochs=None, log=print,
        ckpt_prefix="vit_som"):
    """The Lightning fit loop the reference relies on (train_vit_som.py:86-93), written out.  The best checkpoint is
    <ckpt_dir>/<ckpt_prefix>_<dataset_name>_best.ckpt (train_vit.py:84 names it vit_<dataset>_best)."""
    hp = config["hyperparameters"]
    epochs = int(max_epochs if max_epochs is not None else hp["total_epochs"])
    dev = model.arena.device
    steps_per_epoch = len(train_loader)
    model.set_schedule(len(train_loader.dataset), steps_per_epoch * epochs)     # trainer.estimated_stepping_batches
    (opt,), (sched,) = model.configure_optimizers()
    best_acc, best_path, last_path, history = -1.0, None, None, []
    for epoch in range(epochs):
        model.current_epoch = epoch
        model.train()
        tot, nb = 0.0, 0
        for x, y in train_loader:
            loss = model.train_step_fused(x.to(dev, non_blocking=True), y.to(dev, non_blocking=True))
            opt.step()
            tot, nb = tot + loss, nb + 1                                 # device-side accumulation, no per-step sync
        sched.step()                                                     # LambdaLR, interval = epoch (vit_som.py:159-163)
        rec = {"epoch": epoch, "train/total_loss": float(tot / max(nb, 1)), "lr": opt.param_groups[0]["lr"]}
        if use_validation:
            model.eval()
            correct, seen, vloss, vb = 0.0, 0, 0.0, 0
            for x, y in val_loader:
                x, y = x.to(dev), y.to(dev)
                vloss, vb = vloss + model.validation_step((x, y), vb), vb + 1
                correct, seen = correct + model._last["acc"] * x.shape[0], seen + x.shape[0]
            if model.world_size > 1:                                     # every rank saw 1 / world of the validation set
                agg = torch.stack([torch.as_tensor(correct, dtype=torch.float32, device=dev).reshape(()),
                                   torch.tensor(float(seen), device=dev), torch.as_tensor(vloss, dtype=torch.float32, device=dev).reshape(()),
                                   torch.tensor(float(vb), device=dev)])
                torch.distributed.all_reduce(agg)
                correct, seen, vloss, vb = agg[0], float(agg[1]), agg[2], float(agg[3])
            rec["val/accuracy"] = float(correct / max(seen, 1))
            rec["val/total_loss"] = float(vloss / max(vb, 1))
            if model.rank == 0 and rec["val/accuracy"] > best_acc:        # ModelCheckpoint(monitor='val/accuracy', mode='max')
                best_acc = rec["val/accuracy"]
                best_path = model.save_checkpoint(os.path.join(ckpt_dir, f"{ckpt_prefix}_{dataset_name}_best.ckpt"), opt, sched,
                                                  epoch)
        history.append(rec)
        log(" ".join(f"{k}={v:.5g}" if isinstance(v, float) else f"{k}={v}" for k, v in rec.items()))
    if not use_validation and model.rank == 0:                            # ModelCheckpoint(save_last=True)
        last_path = model.save_checkpoint(os.path.join(ckpt_dir, "last.ckpt"), opt, sched, epochs - 1)
    return {"history": history, "best_model_path": best_path, "last_model_path": last_path, "optimizer": opt}


def _init_process(world, rank, local_rank):
    torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
    if world > 1 and not torch.distributed.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(os.environ.get("VSOM_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    torch.manual_seed(0)                                                  # pl.seed_everything(0)
    np.random.seed(0)


def main_vit(config, n_runs=5, max_epochs=None, make_loaders=synthetic_loaders, model_states_dir="experiments/states/vit",
             log=print):
    """experiments/benchmarking/train_vit.py: the ViT baseline (ViTClassifier).  Each run trains with the best
    val/accuracy checkpointed, reloads that checkpoint and reports the test loader's classification metrics."""
    data_hp = config["data"]
    dataset_name = data_hp["dataset"]
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    _init_process(world, rank, int(os.environ.get("LOCAL_RANK", "0")))
    all_metrics = {k: [] for k in ("accuracy", "precision", "recall", "f1", "run_duration", "inference_time")}
    for run in range(n_runs):
        log(f"Starting run {run + 1} for {dataset_name}...")
        start = time.time()
        if rank == 0:
            clear_directory(model_states_dir)
        train_loader, val_loader, test_loader = make_loaders(config, rank, world)
        log("Training ViT Classifier...")
        model = ViTClassifier(copy.deepcopy(config))
        model.set_distributed(world, rank)
        model.broadcast_parameters()
        fit(model, config, train_loader, val_loader, model_states_dir, dataset_name, True, max_epochs, log, ckpt_prefix="vit")
        model.on_train_end()
        torch.cuda.synchronize()
        run_duration = time.time() - start
        log(f"Run {run + 1} duration: {run_duration:.2f} seconds")
        # rank 0 wrote the best checkpoint (ModelCheckpoint(monitor='val/accuracy', mode='max')); every rank reloads it
        path = os.path.join(model_states_dir, f"vit_{dataset_name}_best.ckpt")
        if world > 1:
            torch.distributed.barrier()
        best_model = ViTClassifier.load_from_checkpoint(path, config=config)
        best_model.set_distributed(world, rank, backend="torch")
        acc, prec, rec, f1, inf_t = evaluate_classification(best_model, config, test_loader)
        for k, v in (("accuracy", acc), ("precision", prec), ("recall", rec), ("f1", f1), ("run_duration", run_duration),
                     ("inference_time", inf_t)):
            all_metrics[k].append(v)
    if n_runs > 1:
        _report(all_metrics, n_runs, dataset_name, log)
    return all_metrics


def main(config, n_runs=5, max_epochs=None, make_loaders=synthetic_loaders, model_states_dir=None, log=print, map_quality=False,
         knn_eval=False, embedding_quality=False, silhouette=False, som_init=None, latent_spectrum=False, som_batch_epochs=0,
         linear_probe=False, tsne_quality=False, map_clusters=False, dbscan_eval=False, spectral_eval=False,
         hdbscan_eval=False, attention_report=False, gmm_eval=False):
    """train_vit_som.py:27-130; a config with hyperparameters.model_arch == "vit" runs main_vit (train_vit.py) instead.
    model_states_dir defaults to experiments/states/vit_som (experiments/states/vit for the ViT baseline).
    map_quality: after each run's final evaluation also run evaluate_map_quality on the training loader with the model that
    was evaluated, and report quantization_error / topographic_error next to the other metrics (ViT-SOM only).
    knn_eval: likewise run evaluate_knn with that model (bank = the training loader, queries = the test loader) and report
    knn_accuracy.
    linear_probe: likewise run evaluate_linear_probe with that model (fitted on the training loader's latents, scored on
    the test loader's) and report linear_probe_accuracy.
    embedding_quality: likewise run evaluate_embedding_quality with that model on the training loader (as map_quality does)
    and report trustworthiness / continuity of the UMAP embedding of its latents.
    tsne_quality: likewise run evaluate_tsne_quality with that model on the training loader and report tsne_trustworthiness
    and tsne_kl of the t-SNE embedding of its latents.
    gmm_eval: likewise run evaluate_gmm with that model on the training loader (a diagonal Gaussian mixture of its latents,
    data.num_classes components) and report gmm_purity, gmm_nmi and gmm_bic.
    map_clusters: likewise run evaluate_map_clusters with that model on the training loader (the SOM's units merged into
    data.num_classes grid-connected clusters, every sample labelled by its BMU's cluster) and report map_cluster_purity and
    map_cluster_nmi: the map's own clustering at the k that gmm_eval and evaluate_kmeans use.
    dbscan_eval: likewise run evaluate_dbscan with that model on the training loader (density clusters of the latents the SOM
    sees, eps from the k-distance curve) and report dbscan_clusters, dbscan_noise, dbscan_purity and dbscan_nmi (the last two
    over the clustered samples only).
    hdbscan_eval: likewise run evaluate_hdbscan with that model on the training loader (density clusters of those latents
    without an eps, chosen by their stability) and report hdbscan_clusters, hdbscan_noise, hdbscan_purity and hdbscan_nmi
    (the last two over the clustered samples only).
    spectral_eval: likewise run evaluate_spectral with that model on the training loader (spectral clustering of the latents'
    kNN graph at data.num_classes clusters) and report spectral_purity, spectral_nmi and spectral_eigengap_k, the number of
    clusters the graph's largest eigengap suggests.
    attention_report: likewise run attention rollout with that model on the training loader (visualize_attention_map, whose
    one loader pass is evaluate_attention's, and visualize_attention_rollout), report rollout_entropy and rollout_cls_mass and
    save the two figures under experiments/plots (a single process only: skipped with a line in the log when world > 1).
    silhouette: likewise run evaluate_silhouette with that model on the training loader, the samples clustered by their
    BMU, and report silhouette_bmu (NaN, with the reason logged, when fewer than two units or every sample alone won).
    som_init: "pca" or "sample": before the first step of each run start the SOM's prototypes from the training loader's
    latents under the fresh encoder (evaluation.init_som_from_data) instead of the uniform random start.
    som_batch_epochs: N > 0: after som_init and before the first step of each run fit the SOM to the training loader's
    latents under the fresh encoder with N epochs of Kohonen's batch map (evaluation.fit_som_batch), and log the
    quantization error before and after; 0 (the default) changes nothing.
    latent_spectrum: after each run also run evaluate_latent_spectrum with the evaluated model on the training loader and
    report effective_rank and components_90 (the components that carry 90% of the variance; NaN when the top 64 do not)."""
    if som_init not in (None, "pca", "sample"):
        raise ValueError(f"som_init must be None, 'pca' or 'sample', got {som_init!r}")
    if int(som_batch_epochs) != som_batch_epochs or som_batch_epochs < 0:
        raise ValueError(f"som_batch_epochs must be a non-negative integer, got {som_batch_epochs!r}")
    if config["hyperparameters"].get("model_arch") == "vit":
        return main_vit(config, n_runs=n_runs, max_epochs=max_epochs, make_loaders=make_loaders,
                        model_states_dir=model_states_dir or "experiments/states/vit", log=log)
    if model_states_dir is None:
        model_states_dir = "experiments/states/vit_som"
    hp, data_hp = config["hyperparameters"], config["data"]
    use_validation = data_hp["num_classes"] > 0
    dataset_name = data_hp["dataset"]
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
    if world > 1 and not torch.distributed.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(os.environ.get("VSOM_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    torch.manual_seed(0)                                                  # pl.seed_everything(0)
    np.random.seed(0)
    all_metrics = {k: [] for k in ("accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time")}
    if map_quality:
        all_metrics.update(quantization_error=[], topographic_error=[])
    if knn_eval:
        all_metrics.update(knn_accuracy=[])
    if linear_probe:
        all_metrics.update(linear_probe_accuracy=[])
    if embedding_quality:
        all_metrics.update(trustworthiness=[], continuity=[])
    if tsne_quality:
        all_metrics.update(tsne_trustworthiness=[], tsne_kl=[])
    if gmm_eval:
        all_metrics.update(gmm_purity=[], gmm_nmi=[], gmm_bic=[])
    if map_clusters:
        all_metrics.update(map_cluster_purity=[], map_cluster_nmi=[])
    if dbscan_eval:
        all_metrics.update(dbscan_clusters=[], dbscan_noise=[], dbscan_purity=[], dbscan_nmi=[])
    if hdbscan_eval:
        all_metrics.update(hdbscan_clusters=[], hdbscan_noise=[], hdbscan_purity=[], hdbscan_nmi=[])
    if spectral_eval:
        all_metrics.update(spectral_purity=[], spectral_nmi=[], spectral_eigengap_k=[])
    if attention_report:
        all_metrics.update(rollout_entropy=[], rollout_cls_mass=[])
    if silhouette:
        all_metrics.update(silhouette_bmu=[])
    if latent_spectrum:
        all_metrics.update(effective_rank=[], components_90=[])
    for run in range(n_runs):
        log(f"Starting run {run + 1} for {dataset_name}...")
        start = time.time()
        if rank == 0:
            clear_directory(model_states_dir)
        train_loader, val_loader, test_loader = make_loaders(config, rank, world)
        model = ViTSOM(copy.deepcopy(config))
        model.set_distributed(world, rank)
        model.broadcast_parameters()                                      # DDP broadcasts rank 0's weights at construction
        if som_init:
            fitted = init_som_from_data(model, config, train_loader, method=som_init)
            log(f"SOM initialised from the training latents ({som_init}"
                + (f", PC1+PC2 carry {float(fitted.explained_variance_ratio_.sum()):.3f} of the variance)" if fitted is not None else ")"))
        if som_batch_epochs:
            br = fit_som_batch(model, config, train_loader, epochs=int(som_batch_epochs))
            log(f"SOM batch map: {int(som_batch_epochs)} epochs, quantization error {float(br.quantization_error[0]):.4f} before, "
                f"{br.final_quantization_error:.4f} after, dead units {br.dead_units}/{br.hits.size}")
        out = fit(model, config, train_loader, val_loader, model_states_dir, dataset_name, use_validation, max_epochs, log)
        torch.cuda.synchronize()
        run_duration = time.time() - start
        log(f"Run {run + 1} duration: {run_duration:.2f} seconds")
        # Final evaluation: every rank folds ITS shard of the loader into the contingency table and the tables are summed
        # over the ranks (evaluation.py), so all ranks hold the metrics of the whole set.
        if use_validation:
            acc, prec, rec, f1, inf_t = evaluate_classification(model, config, test_loader)
            for k, v in (("accuracy", acc), ("precision", prec), ("recall", rec), ("f1", f1)):
                all_metrics[k].append(v)
            evaluated = model
        else:
            # the reference reloads the last checkpoint (train_vit_som.py:111): rank 0 wrote it, every rank loads that file
            path = os.path.join(model_states_dir, "last.ckpt")
            if world > 1:
                torch.distributed.barrier()
            final_model = ViTSOM.load_from_checkpoint(path, config=config)
            final_model.set_distributed(world, rank, backend="torch")
            purity, nmi, inf_t = evaluate_clustering(final_model, config, train_loader)
            all_metrics["purity"].append(purity)
            all_metrics["nmi"].append(nmi)
            evaluated = final_model
        if map_quality:
            mq = evaluate_map_quality(evaluated, config, train_loader)
            log(f"Map quality: quantization error {mq.quantization_error:.4f}, topographic error {mq.topographic_error:.4f}, "
                f"dead units {mq.dead_units}/{mq.hits.size}")
            all_metrics["quantization_error"].append(mq.quantization_error)
            all_metrics["topographic_error"].append(mq.topographic_error)
        if knn_eval:
            kr = evaluate_knn(evaluated, config, train_loader, test_loader)
            log(f"kNN probe: accuracy {kr.accuracy:.4f} (k={kr.k}, {kr.n_train} training / {kr.n_test} test samples)")
            all_metrics["knn_accuracy"].append(kr.accuracy)
        if linear_probe:
            lp = evaluate_linear_probe(evaluated, config, train_loader, test_loader)
            log(f"Linear probe: accuracy {lp.accuracy:.4f} (train {lp.train_accuracy:.4f}, {lp.n_iter} iterations, "
                f"{'converged' if lp.converged else 'not converged'}, {lp.n_train} training / {lp.n_test} test samples)")
            all_metrics["linear_probe_accuracy"].append(lp.accuracy)
        if embedding_quality:
            eq = evaluate_embedding_quality(evaluated, config, train_loader)
            log(f"Embedding quality: trustworthiness {eq.trustworthiness:.4f}, continuity {eq.continuity:.4f} "
                f"(k={eq.n_neighbors}, {eq.n_samples} samples)")
            all_metrics["trustworthiness"].append(eq.trustworthiness)
            all_metrics["continuity"].append(eq.continuity)
        if tsne_quality:
            tq = evaluate_tsne_quality(evaluated, config, train_loader)
            log(f"t-SNE quality: trustworthiness {tq.trustworthiness:.4f}, continuity {tq.continuity:.4f}, KL {tq.kl_divergence:.4f} "
                f"(k={tq.n_neighbors}, {tq.n_samples} samples)")
            all_metrics["tsne_trustworthiness"].append(tq.trustworthiness)
            all_metrics["tsne_kl"].append(tq.kl_divergence)
        if gmm_eval:
            gr = evaluate_gmm(evaluated, config, train_loader)
            log(f"Gaussian mixture: purity {gr.purity:.4f}, NMI {gr.nmi:.4f}, BIC {gr.bic:.1f}, mean log-likelihood "
                f"{gr.log_likelihood:.3f} ({gr.n_components} components, {gr.n_iter} iterations, {gr.n_samples} samples)")
            all_metrics["gmm_purity"].append(gr.purity)
            all_metrics["gmm_nmi"].append(gr.nmi)
            all_metrics["gmm_bic"].append(gr.bic)
        if map_clusters:
            mc = evaluate_map_clusters(evaluated, config, train_loader)
            log(f"Map clusters: purity {mc.purity:.4f}, NMI {mc.nmi:.4f} ({mc.n_clusters} clusters of {mc.unit_labels.numel()} units, "
                f"{mc.linkage} linkage, {mc.metric}, {mc.n_samples} samples)")
            all_metrics["map_cluster_purity"].append(mc.purity)
            all_metrics["map_cluster_nmi"].append(mc.nmi)
        if dbscan_eval:
            dr = evaluate_dbscan(evaluated, config, train_loader)
            log(f"DBSCAN: {dr.n_clusters} clusters, {dr.n_noise} noise rows of {dr.n_samples} (coverage {dr.coverage:.3f}), purity "
                f"{dr.purity:.4f}, NMI {dr.nmi:.4f} (eps {dr.eps:.6g}, min_samples {dr.min_samples}, {dr.metric})")
            all_metrics["dbscan_clusters"].append(float(dr.n_clusters))
            all_metrics["dbscan_noise"].append(float(dr.n_noise))
            all_metrics["dbscan_purity"].append(dr.purity)
            all_metrics["dbscan_nmi"].append(dr.nmi)
        if hdbscan_eval:
            hr = evaluate_hdbscan(evaluated, config, train_loader)
            log(f"HDBSCAN: {hr.n_clusters} clusters, {hr.n_noise} noise rows of {hr.n_samples} (coverage {hr.coverage:.3f}), purity "
                f"{hr.purity:.4f}, NMI {hr.nmi:.4f} (min_cluster_size {hr.min_cluster_size}, min_samples {hr.min_samples}, {hr.metric}, "
                f"{hr.n_rounds} rounds)")
            all_metrics["hdbscan_clusters"].append(float(hr.n_clusters))
            all_metrics["hdbscan_noise"].append(float(hr.n_noise))
            all_metrics["hdbscan_purity"].append(hr.purity)
            all_metrics["hdbscan_nmi"].append(hr.nmi)
        if spectral_eval:
            sr = evaluate_spectral(evaluated, config, train_loader)
            log(f"Spectral clustering: purity {sr.purity:.4f}, NMI {sr.nmi:.4f} at k {sr.n_clusters}; the eigengap suggests k "
                f"{sr.eigengap_k}; {sr.n_connected_components} graph components, {sr.n_iter} passes ({sr.metric}, "
                f"{sr.n_neighbors} neighbours)")
            all_metrics["spectral_purity"].append(sr.purity)
            all_metrics["spectral_nmi"].append(sr.nmi)
            all_metrics["spectral_eigengap_k"].append(float(sr.eigengap_k))
        if attention_report:
            if world > 1:
                log("Attention rollout: skipped (evaluate_attention runs in a single process only)")
            else:
                ar, map_path = visualize_attention_map(evaluated, config, train_loader)
                _, roll_path = visualize_attention_rollout(evaluated, config, train_loader)
                log(f"Attention rollout: rollout_entropy {ar.entropy:.4f}, rollout_cls_mass {ar.cls_mass:.4f} ({ar.head_fusion} fusion, "
                    f"residual {ar.residual:g}, query {ar.query!r}, {ar.n_samples} samples); figures: {map_path}, {roll_path}")
                all_metrics["rollout_entropy"].append(ar.entropy)
                all_metrics["rollout_cls_mass"].append(ar.cls_mass)
        if silhouette:
            try:
                sr = evaluate_silhouette(evaluated, config, train_loader, clusters="bmu")
                log(f"Silhouette: silhouette_bmu {sr.score:.4f} ({sr.metric}, {int((sr.counts > 0).sum())} of {sr.n_clusters} units "
                    f"hit, {sr.n_samples} samples)")
                all_metrics["silhouette_bmu"].append(sr.score)
            except ValueError as err:
                if "Number of labels" not in str(err):     # sklearn's rule: 2 .. n_samples - 1 clusters; anything else is an error
                    raise
                log(f"Silhouette: silhouette_bmu undefined ({err})")
                all_metrics["silhouette_bmu"].append(float("nan"))
        if latent_spectrum:
            ls = evaluate_latent_spectrum(evaluated, config, train_loader)
            c90 = ls.components_for[0.9]
            log(f"Latent spectrum: effective_rank {ls.effective_rank:.2f} of the top {len(ls.explained_variance)}, "
                f"components_90 {c90} ({ls.n_samples} samples)")
            all_metrics["effective_rank"].append(ls.effective_rank)
            all_metrics["components_90"].append(float("nan") if c90 is None else float(c90))
        all_metrics["run_duration"].append(run_duration)
        all_metrics["inference_time"].append(inf_t)
    if n_runs > 1:
        _report(all_metrics, n_runs, dataset_name, log)
    return all_metrics


def _parser():
    ap = argparse.ArgumentParser(description="ViT-SOM / ViT training driver (MI355X)")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--device-data", action="store_true", help="keep the data on the GPU as uint8 and augment it there")
    ap.add_argument("--data-npz", type=str, default=None, help="a local .npz with images / labels (implies --device-data)")
    ap.add_argument("--device-randaug", action="store_true",
                    help="also apply the config's RandAugment / timm rand-m9 auto-augment on the GPU (implies --device-data)")
    ap.add_argument("--map-quality", action="store_true",
                    help="after each run also report the map's quantization and topographic error on the training set")
    ap.add_argument("--knn-eval", action="store_true",
                    help="after each run also report the k-nearest-neighbour accuracy of the latents (bank: training set, queries: test set)")
    ap.add_argument("--linear-probe", action="store_true",
                    help="after each run also report the accuracy of a linear classifier fitted on the frozen latents (fit: training "
                         "set, scored: test set)")
    ap.add_argument("--embedding-quality", action="store_true",
                    help="after each run also report trustworthiness and continuity of the UMAP embedding of the training set's latents")
    ap.add_argument("--tsne-quality", action="store_true",
                    help="after each run also report trustworthiness and KL divergence of the t-SNE embedding of the training set's latents")
    ap.add_argument("--gmm-eval", action="store_true",
                    help="after each run also report purity, NMI and BIC of a diagonal Gaussian mixture fitted on the training set's latents")
    ap.add_argument("--map-clusters", action="store_true",
                    help="after each run also report purity and NMI of the SOM's units merged into data.num_classes grid-connected "
                         "clusters (agglomerative clustering of the prototypes), every sample labelled by its BMU's cluster")
    ap.add_argument("--spectral-eval", action="store_true",
                    help="after each run also report spectral clustering of the training set's latents (kNN graph, data.num_classes "
                         "clusters): purity, NMI and the number of clusters the largest eigengap suggests")
    ap.add_argument("--dbscan-eval", action="store_true",
                    help="after each run also report the density clusters (DBSCAN) of the training set's latents: clusters, noise rows, "
                         "purity and NMI over the clustered samples")
    ap.add_argument("--attention-report", action="store_true",
                    help="after each run also report attention rollout of the encoder on the training set (rollout_entropy, "
                         "rollout_cls_mass) and save the per-image overlay and the per-unit / per-class attention maps")
    ap.add_argument("--hdbscan-eval", action="store_true",
                    help="after each run also report the density clusters without an eps (HDBSCAN) of the training set's latents: "
                         "clusters, noise rows, purity and NMI over the clustered samples")
    ap.add_argument("--silhouette", action="store_true",
                    help="after each run also report the silhouette coefficient of the training set's latents clustered by their BMU")
    ap.add_argument("--som-init", choices=("pca", "sample"), default=None,
                    help="start the SOM's prototypes from the training set's latents: the plane of their first two principal "
                         "components (pca) or random samples (sample), instead of the uniform random start")
    ap.add_argument("--som-batch-epochs", type=int, default=0, metavar="N",
                    help="before the first step (after --som-init) fit the SOM to the training set's latents with N epochs of "
                         "Kohonen's batch map")
    ap.add_argument("--latent-spectrum", action="store_true",
                    help="after each run also report the effective rank of the training set's latents and the number of principal "
                         "components that carry 90%% of their variance")
    return ap


if __name__ == "__main__":
    a = _parser().parse_args()
    loaders = synthetic_loaders
    if a.device_data or a.data_npz or a.device_randaug:
        loaders = lambda c, r, w: device_loaders(c, r, w, npz=a.data_npz, auto_augment=a.device_randaug)     # noqa: E731
    main(load_config(a.config), n_runs=a.runs, max_epochs=a.epochs, make_loaders=loaders, map_quality=a.map_quality,
         knn_eval=a.knn_eval, embedding_quality=a.embedding_quality, silhouette=a.silhouette, som_init=a.som_init,
         latent_spectrum=a.latent_spectrum, som_batch_epochs=a.som_batch_epochs, linear_probe=a.linear_probe,
         tsne_quality=a.tsne_quality, gmm_eval=a.gmm_eval, map_clusters=a.map_clusters, dbscan_eval=a.dbscan_eval,
         spectral_eval=a.spectral_eval, hdbscan_eval=a.hdbscan_eval, attention_report=a.attention_report)
