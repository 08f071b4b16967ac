"""experiment() — the reference's single entry point (itexperiments.py:42-605), re-provided with the
same keyword surface so that examples/simple_example.py-style calls run unchanged, with the model
forward/backward executing in the HIP message-passing kernels.

Scope: data loading / mask remake / feature normalisation / model dispatch by
lower-cased ``model_name`` / full-batch Adam + NLLLoss loop with early stopping / the PTA branch
(label propagation + soft-label loss + propagated inference, reference :351-374, :422-462) / metrics
dict / Correct & Smooth post-processing (reference :514-534). Out of scope and rejected with
``NotImplementedError``: plots, PCA (reference :536-601) and the FAGCN zoo member. SuperGAT trains on
``NLL + supergat_graph_lambda * att_loss`` (reference :431-432), on the eager loop.

Deliberate deviations from reference quirks:
  * ``compare_pred_label(need_all_metrics=False)`` returns zeros instead of raising
    ``UnboundLocalError`` (reference :658-664).

Same results by default, fix as an opt-in: with ``specify_data=True`` the reference ALWAYS remakes the masks — its
test ``(not valid_list) or (not valid_tensor)`` (:210) is true for every input, masks cannot be lists and tensors at
once — and so does this function. ``keep_valid_data_mask=True`` (an addition) applies the test the code was
evidently meant to make, ``not (valid_list or valid_tensor)``, and keeps supplied masks that pass it.
"""
import inspect
import os
import random
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .data import Data
from .initial_params import InitialParameters
from .models import MODELS
from .rd2pd import RD2PD
from .utils import get_classification_mask, get_random_mask, get_whole_mask, to_undirected

_OUT_OF_SCOPE = ("fagcn",)


def _macro_prf(label, pred):
    """Macro precision / recall / F1 and micro F1 with zero_division=0, over the labels present in
    either vector (what sklearn.metrics computes at reference :653-657)."""
    try:
        from sklearn import metrics
        return (metrics.precision_score(label, pred, average="macro", zero_division=0),
                metrics.recall_score(label, pred, average="macro", zero_division=0),
                metrics.f1_score(label, pred, average="macro", zero_division=0),
                metrics.f1_score(label, pred, average="micro", zero_division=0))
    except ImportError:  # same arithmetic without sklearn
        label, pred = np.asarray(label), np.asarray(pred)
        classes = np.union1d(label, pred)
        p, r, f = [], [], []
        for c in classes:
            tp = float(np.sum((pred == c) & (label == c)))
            pp, ap = float(np.sum(pred == c)), float(np.sum(label == c))
            pc = tp / pp if pp else 0.0
            rc = tp / ap if ap else 0.0
            p.append(pc)
            r.append(rc)
            f.append(2 * pc * rc / (pc + rc) if pc + rc else 0.0)
        micro = float(np.mean(pred == label)) if len(label) else 0.0
        return float(np.mean(p)), float(np.mean(r)), float(np.mean(f)), micro


def compare_pred_label(pred, label, need_all_metrics):
    """Accuracy (+ macro precision/recall/F1, micro F1) of two label vectors (reference :639-664)."""
    total = pred.size(0)
    accuracy = pred.eq(label).sum().item() / total
    precision = recall = f1_macro = f1_micro = 0
    if need_all_metrics:
        p = pred.cpu() if isinstance(pred, Tensor) else pred
        l = label.cpu() if isinstance(label, Tensor) else label
        precision, recall, f1_macro, f1_micro = _macro_prf(l, p)
    return {"ACC": accuracy, "precision_score": precision, "recall_score": recall,
            "f1_macro": f1_macro, "f1_micro": f1_micro}


def test(model, x, y, mask, need_all_metrics):
    """Eval-mode forward + metrics on `mask` (reference :611-634). `x` = forward kwargs dict."""
    model.eval()
    with torch.no_grad():
        pure_out = model(**x)
    out = pure_out["out"]
    pred = out.max(dim=1)[1][mask]
    label = y[mask]
    res = compare_pred_label(pred, label, need_all_metrics)
    res.update({"test_op": out, "pred": pred, "label": label, "emb": pure_out["emb"], "pure_out": pure_out})
    return res


def _normalize_features(features, how, method):
    """reference :261-299: 'row' / 'col' / 'all' x MinMaxScalar / StandardScalar / sum."""
    dim = {"row": 1, "col": 0, "all": [0, 1]}[how]
    if method == "MinMaxScalar":
        if isinstance(dim, int):
            lo, hi = torch.min(features, dim)[0], torch.max(features, dim)[0]
        else:
            lo, hi = torch.min(features), torch.max(features)
        den = (hi - lo).clamp(min=1e-12)
        return ((features.T - lo) / den).T if dim == 1 else (features - lo) / den
    if method == "StandardScalar":
        mean, std = torch.mean(features, dim), torch.std(features, dim)
        den = std.clamp(min=1e-12)
        return ((features.T - mean) / den).T if dim == 1 else (features - mean) / den
    return features / features.sum(dim, keepdim=True).clamp(min=1)


def _masks_usable(data):
    """Masks exist and are index lists or 1-D tensors no longer than the node count (reference
    :196-209)."""
    names = ("train_mask", "val_mask", "test_mask")
    if not all(getattr(data, n, None) is not None for n in names):
        return False
    n = data.num_nodes
    ms = [getattr(data, k) for k in names]
    if all(isinstance(m, list) for m in ms):
        return all(len(m) <= n for m in ms)
    if all(isinstance(m, Tensor) for m in ms):
        return all(m.dim() == 1 and m.size(0) <= n for m in ms)
    return False


def _must_remake_masks(data, remake_data_mask, keep_valid_data_mask):
    """reference :210 `remake_data_mask or (not mask_exist) or (not valid_list) or (not valid_tensor)`: the last two
    terms cannot both be false, so the reference remakes the masks of a supplied `data` on every call. The default
    here is that behaviour; keep_valid_data_mask=True (opt-in fix) keeps masks that exist and are valid."""
    if remake_data_mask or not keep_valid_data_mask:
        return True
    return not _masks_usable(data)


def _as_bool_mask(mask, n, device):
    """The reference accepts masks as index lists, index tensors or boolean tensors (:193-209); the loop
    works on boolean masks of length N."""
    if isinstance(mask, Tensor) and mask.dtype == torch.bool and mask.numel() == n:
        return mask.to(device)
    idx = torch.as_tensor(mask, dtype=torch.long, device=device) if not isinstance(mask, Tensor) else mask.to(device)
    if idx.dtype == torch.bool:  # shorter boolean mask: pad with False
        out = torch.zeros(n, dtype=torch.bool, device=device)
        out[:idx.numel()] = idx
        return out
    out = torch.zeros(n, dtype=torch.bool, device=device)
    out[idx.long()] = True
    return out


def _make_masks(y, mode, ratio, num_train_per_class, num_val, num_test, seed):
    if mode == "ratio":
        return get_whole_mask(y, ratio, seed)
    if mode == "classification":
        return get_classification_mask(y, ratio, seed)
    if mode == "random":
        return get_random_mask(y, num_train_per_class, num_val, num_test, seed)
    raise ValueError(f"dataset_split_mode {mode!r} not in ratio/classification/random")


def normalized_adjacency(edge_index, num_nodes):
    """reference :354-357 (edge_index2sparse_matrix + I, normalize_adj): D^-1/2 (A + I) D^-1/2 with
    adj[src, dst], as a device-resident CSR (models.pta.NormAdj) instead of a torch sparse tensor."""
    from .models.pta import NormAdj
    return NormAdj(edge_index, num_nodes)


def label_propagation(adj, labels, idx, K, alpha, device=None):
    """reference :698-719: K rounds of y <- adj @ y, clamp the rows in `idx` to their one-hot labels,
    y <- (1-alpha) y + alpha y0."""
    n_class = int(labels.max().item()) + 1
    y0 = torch.zeros((labels.shape[0], n_class), dtype=torch.float32, device=labels.device)
    y0[idx, labels[idx]] = 1.0
    onehot = torch.nn.functional.one_hot(labels.clamp(min=0), n_class).to(torch.float32)
    y = y0
    for _ in range(K):
        y = adj.matmul(y)
        y[idx] = onehot[idx]
        y = (1 - alpha) * y + alpha * y0
    return y


_EDGE_WEIGHT_MODELS = ("gcn", "appnpstack", "sgc")  # experiment(use_edge_weight=True)

# use_hip_graph=True captures the epoch only up to this many edges: beyond it the aggregation kernels, not launch
# latency, set the epoch time, and a replayed graph was measured slower
HIP_GRAPH_MAX_EDGES = 20_000_000


def experiment(model_init_param: dict, *,
               task: str = "node_prediction",
               dataset_name: str = "Github",
               dataset_root: str = InitialParameters.default_data_path,
               dataset_split_mode: str = "ratio",
               dataset_split_ratio: str = "6-2-2",
               num_train_per_class: int = 20, num_val: int = 500, num_test: int = 1000,
               dataset_split_seed: int = 123456789,
               specify_data: bool = False, data: Data = None, remake_data_mask: bool = False,
               keep_valid_data_mask: bool = False,
               to_undirected_graph: bool = False,
               normalize_feature: str = None, normalize_feature_method: str = None,
               pta_loss_decay: float = 0.05,
               pta_weight_decay: float = 0.005,
               supergat_graph_lambda: float = 4,
               cuda_index: int = 0, use_cpu: bool = False,
               need_to_reappear: bool = False, reappear_seed: int = 14530529,
               model_name: str = "MLP",
               learning_rate: float = 0.1, weight_decay: float = 0,
               epoch: int = 50,
               early_stopping: int = 10,
               early_stopping_criterion: str = "acc",
               implement_early_stopping: bool = True,
               post_cs: bool = False,
               cs_param: dict = None,
               print_pics: bool = False,
               pics_root: str = InitialParameters.default_pics_path,
               pics_name: str = "pic1.png",
               print_confusion_matrix: bool = False,
               check_data_valid: bool = False,
               vis_feat: bool = False,
               feat_pic_names_prefix: str = None,
               total_seed: int = 12345678,
               ini_seed: int = 1234567,
               need_all_metrics: bool = True,
               f1_average: str = "macro",
               loss_func_hp: dict = None, print_print: bool = True,
               specify_model: bool = True, model: nn.Module = None,
               begin_early_stopping: int = 20,
               return_model: bool = False,
               use_hip_graph: bool = True,
               share_eval_forward: bool = True,
               cache_input_aggregate="auto",
               distributed=None,
               task_split: str = "auto",
               use_edge_weight: bool = False,
               use_edge_attr: bool = False,
               use_edge_type: bool = False,
               num_neighbors=None,
               batch_size: int = 1024):
    """Train + evaluate one model on one graph; returns {'ACC', 'precision_score', 'recall_score',
    'f1_macro', 'f1_micro'} (reference :603-605). ``return_model=True`` (an addition) also returns
    the trained module and the per-epoch curves under 'model' / 'history'. ``use_hip_graph=True`` (an
    addition) captures one epoch of the loop into a hipGraph and replays it (epoch_graph.py); the
    arithmetic is unchanged, only launch latency and host round-trips go away; on graphs beyond
    ``HIP_GRAPH_MAX_EDGES`` edges, where the kernels and not the launches set the epoch time (replay measured 3 %
    faster at 4 M edges, 4 % slower at 60 M), the eager loop runs instead unless ``use_hip_graph="always"``.
    ``share_eval_forward`` (an addition, ON by default since round 4: results are bit-identical,
    test_shared_eval_forward_changes_nothing_but_the_forward_count) takes the per-epoch test metrics from the val pass's
    eval-mode outputs instead of running the reference's second, identical eval forward (itexperiments.py:464-473): same
    numbers, two forwards per epoch instead of three; ``False`` forwards twice as the reference does.
    ``cache_input_aggregate`` (an addition; "auto" = on when HBM allows, also bit-identical,
    test_cached_input_aggregate_changes_nothing_but_the_aggregation_count) keeps the first conv layer's aggregate of
    the input features — the same matrix in every forward of every epoch, because features and graph are static
    (itexperiments.py:417-473 recomputes it three times per epoch) — so that together with the shared eval forward a
    2-layer GCN / GraphSAGE epoch runs 3 aggregations instead of 7; models whose first layer has no aggregate-first
    form (in > out) ignore it; "auto" turns it off when the kept [N, F] matrix would take more than a quarter of the free
    HBM (the memory guard); ``True`` / ``False`` force it. ``distributed`` (an addition; the reference is single-device, :246): None = take the
    node-partitioned route when the script runs as one of several ranks (``torchrun --nproc-per-node N script.py``:
    WORLD_SIZE > 1 in the environment, one process per GPU, device = LOCAL_RANK); every rank calls experiment() with
    the same arguments and the same data and gets the same result dict. Models: gcn / graphsage / graphsage2 / gat /
    appnpstack (rgb_experiment_amd.dist.DistRunner); no hipGraph, no post_cs there. ``task_split`` (distributed runs):
    "auto" | "on" | "off" — whether the epoch is split by task over two groups of ranks (dist/tasksplit.py). On TWO ranks
    the split puts the WHOLE graph on both GPUs (one trains, one evaluates: fastest, but no memory scaling): "auto" takes
    it only when one GPU can hold the whole graph and falls back to the node partition (half of everything per rank)
    otherwise; "off" always partitions; the environment variable RGBX_TASK_SPLIT overrides "auto".
    ``model`` (declared and never read by the reference, :78; live here): a ``nn.Module`` to train INSTEAD of building one
    from ``model_name``. ``model_init_param`` is then ignored and ``model_name`` is only the label of the log line (it
    still passes the out-of-scope / unknown-name checks). The module is moved to the run's device; its forward takes
    ``x`` (and ``edge_index`` when its signature has one) and returns a mapping with 'out' and 'emb' (ValueError
    before the loop otherwise); it runs on the generic loop — loss and accuracy from its logits (ops.ce_from_logits /
    ops.masked_ce_accuracy) — single-device, with ``use_hip_graph`` honoured as for any model. ``use_cpu=True`` is not
    refused up front: a module that owns a graph layer raises that layer's "no CPU fallback" RuntimeError. This is how
    FAGCN trains (``model=rgb_experiment_amd.models.FAGCN(...)``) while the NAME "fagcn" stays refused. ``model=None``
    (default) changes nothing. ``use_edge_weight=True`` (an addition, off by default): ``data.edge_weight`` (float [E])
    goes to the device with the data and into the forward arguments as ``edge_weight`` — gcn_norm's parameter
    (models/dagnn.py:12-31) — for the four routes that take weights: ``gcn``, ``appnpstack``, ``sgc`` and ``post_cs``
    (any other model_name: ValueError). Not with ``to_undirected_graph`` (the reference's to_undirected call carries no
    weights: ValueError) and not on the partitioned route (NotImplementedError). With the flag off a ``Data`` that
    happens to carry an ``edge_weight`` attribute behaves exactly as one without. ``use_edge_attr=True`` (an addition, off by
    default): ``data.edge_attr`` (float [E, D], one feature row per edge) goes to the device with the data and into the
    forward arguments as ``edge_attr``, for ``model_name="gine"`` (models.GINE, built with ``edge_dim`` in
    ``model_init_param``), for ``model_name="monet"`` (models.MoNet, built with ``kernel_size`` and ``dim`` = D; without the
    flag it runs on the degree pseudo-coordinates of the graph), for ``model_name="pna"`` (models.PNA, built with ``edge_dim``
    = D; without the flag, and with ``edge_dim`` left out, it runs on the node features alone), for ``model_name="cgcnn"``
    (models.CGCNN, built with ``edge_dim`` = D; without the flag, and with ``edge_dim`` = 0, it runs on the node features
    alone) and for a caller's ``model=`` whose forward takes
    ``edge_attr`` (any other model_name: ValueError). Not with ``to_undirected_graph`` (that call carries no attributes: ValueError) and not on the partitioned
    route (NotImplementedError). With the flag off a ``Data`` that happens to carry an ``edge_attr`` behaves exactly as
    one without (``gine`` then fails at its forward, which needs the argument). ``use_edge_type=True`` (an addition, off by
    default): ``data.edge_type`` (int64 [E], one relation per edge) goes to the device with the data and into the forward
    arguments as ``edge_type``, for ``model_name="rgcn"`` (models.RGCN, built with ``num_relations`` and optionally
    ``num_bases`` in ``model_init_param``), for ``model_name="film"`` (models.FiLM, built with ``num_relations``; without
    the flag it runs with one relation) and for a caller's ``model=`` whose forward takes ``edge_type`` (any other
    model_name: ValueError). Not with ``to_undirected_graph`` (that call carries no types: ValueError) and not on the
    partitioned route (NotImplementedError). With the flag off a ``Data`` that happens to carry an ``edge_type`` behaves
    exactly as one without. ``num_neighbors`` (an addition; None, the default, changes nothing): a non-empty list of
    fan-outs, each >= 1 or -1 for all neighbours, turns the TRAINING side of every epoch into neighbour-sampled
    mini-batches (rgb_experiment_amd.NeighborSampler, drawn by HIP kernels): the training rows are permuted, cut into
    batches of ``batch_size`` seeds, and each batch is sampled (hop h draws ``num_neighbors[h]`` in-edges of the nodes hop
    h - 1 brought in), its feature rows and labels are gathered, the model's training forward runs on the batch's
    ``(x, edge_index)``, the loss and the train accuracy are taken on its seed rows (the same masked cross-entropy as the
    full-batch loop), followed by backward and ONE optimizer step per batch; the epoch's ``history`` entries are the
    seed-weighted means over its batches. Validation and test forwards stay full-graph. The route runs eagerly
    (``use_hip_graph`` is ignored: shapes change per batch) and ``cache_input_aggregate`` is off on it (a kept
    whole-graph aggregate must never reach a batch forward). Layers that normalise by the source's degree (``GCNConv``'s
    ``gcn_norm``) see the BATCH's degrees at its outer ring, as in PyG, and so are not exact there; layers that normalise by
    the target only (mean or sum SAGE, GIN, the attention families) are exact on the seeds once there are as many hops as
    layers and all fan-outs are -1. Refused before any device work: a malformed ``num_neighbors`` or ``batch_size`` < 1
    (ValueError), ``model_name="pta"`` (ValueError), a layer that keeps its first call's propagated features —
    ``SGConv(cached=True)``, the default of ``model_name="sgc"``: pass ``cached=False`` in ``model_init_param``; also looked for
    in a caller's ``model=`` — (ValueError: the kept rows of the first batch would meet every other batch and the full-graph
    evaluation), ``use_edge_weight`` / ``use_edge_attr`` / ``use_edge_type`` (ValueError:
    the batch's ``e_id`` is what a later change needs for them) and the partitioned route (NotImplementedError)."""
    say = print if print_print else (lambda *a, **k: None)
    say(f"running node classification: {'custom' if specify_data else dataset_name} data, model {model_name}")

    name = model_name.lower()
    if name in _OUT_OF_SCOPE:
        raise NotImplementedError(f"model_name={model_name!r} is outside the MI355X hot-path scope "
                                  f"(supported: {sorted(MODELS)})")
    if name not in MODELS:
        raise ValueError(f"unknown model_name {model_name!r}")
    if print_pics or vis_feat:
        raise NotImplementedError("print_pics / vis_feat are reporting features outside the hot-path scope")
    if post_cs and name == "pta":
        raise ValueError("post_cs cannot be combined with PTA (reference :517)")
    if num_neighbors is not None:
        from .sampler import check_num_neighbors
        num_neighbors = check_num_neighbors(num_neighbors)
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"batch_size must be an int >= 1, got {batch_size!r}")
        if name == "pta" and model is None:
            raise ValueError("num_neighbors: PTA trains on labels propagated over the whole graph; it has no sampled form")
        if use_edge_weight or use_edge_attr or use_edge_type:
            raise ValueError("num_neighbors cannot be combined with use_edge_weight / use_edge_attr / use_edge_type yet "
                             "(the sampled batch's e_id is what gathers them)")
        # a layer that keeps its propagated features after the first call (SGConv(cached=True), SGC's default) would
        # serve the first batch's rows to every later batch and to the full-graph evaluation
        keeps = ([type(m).__name__ for m in model.modules() if getattr(m, "cached", False)]
                 if isinstance(model, nn.Module) else
                 ["SGConv"] if name == "sgc" and model is None and (model_init_param or {}).get("cached", True) else [])
        if keeps:
            raise ValueError(f"num_neighbors: {keeps[0]}(cached=True) keeps the first call's propagated features, which "
                             "must never meet another batch or the full graph; build it with cached=False "
                             "(model_name='sgc': model_init_param['cached'] = False)")
    if use_edge_weight:
        if name not in _EDGE_WEIGHT_MODELS or model is not None:
            raise ValueError(f"use_edge_weight=True: model_name={model_name!r} takes no edge weights; the routes that do "
                             "are gcn, appnpstack, sgc and post_cs (on one of those three models)")
        if to_undirected_graph:
            raise ValueError("use_edge_weight=True cannot be combined with to_undirected_graph=True: the reference's "
                             "to_undirected call (:235-238) carries no weights")

    if use_edge_attr:
        if model is not None:
            if not isinstance(model, nn.Module) or "edge_attr" not in inspect.signature(model.forward).parameters:
                raise ValueError("use_edge_attr=True: the forward of the module passed as model= takes no edge_attr")
        elif name not in ("gine", "monet", "pna", "cgcnn"):
            raise ValueError(f"use_edge_attr=True: model_name={model_name!r} takes no edge attributes; the routes that do "
                             "are gine, monet, pna, cgcnn and a model= whose forward takes edge_attr")
        if to_undirected_graph:
            raise ValueError("use_edge_attr=True cannot be combined with to_undirected_graph=True: the reference's "
                             "to_undirected call (:235-238) carries no attributes")

    if use_edge_type:
        if model is not None:
            if not isinstance(model, nn.Module) or "edge_type" not in inspect.signature(model.forward).parameters:
                raise ValueError("use_edge_type=True: the forward of the module passed as model= takes no edge_type")
        elif name not in ("rgcn", "film"):
            raise ValueError(f"use_edge_type=True: model_name={model_name!r} takes no edge types; the routes that do "
                             "are rgcn, film and a model= whose forward takes edge_type")
        if to_undirected_graph:
            raise ValueError("use_edge_type=True cannot be combined with to_undirected_graph=True: the reference's "
                             "to_undirected call (:235-238) carries no types")

    # ---- data (reference :179-229) ----------------------------------------------------------
    if not specify_data:
        data = RD2PD(dataset_root=dataset_root, dataset_name=dataset_name, split_method=dataset_split_mode,
                     split_ratio=dataset_split_ratio, split_seed=dataset_split_seed,
                     num_train_per_class=num_train_per_class, num_val=num_val, num_test=num_test).data
    else:
        data = data.clone()
        if _must_remake_masks(data, remake_data_mask, keep_valid_data_mask):
            say("re-splitting the dataset (train/val/test masks)")
            data.train_mask, data.val_mask, data.test_mask = _make_masks(
                data.y.cpu(), dataset_split_mode, dataset_split_ratio, num_train_per_class, num_val, num_test,
                dataset_split_seed)

    if use_edge_attr:  # the contract of data.edge_attr, checked before any device is touched
        edge_attr = getattr(data, "edge_attr", None)
        if not torch.is_tensor(edge_attr) or not edge_attr.is_floating_point():
            raise ValueError("use_edge_attr=True needs data.edge_attr: a float tensor of shape [E, D]")
        if edge_attr.dim() != 2 or edge_attr.size(0) != data.edge_index.size(1):
            raise ValueError(f"data.edge_attr must have shape [E, D] = [{data.edge_index.size(1)}, D], got "
                             f"{tuple(edge_attr.shape)}")

    if use_edge_type:  # the contract of data.edge_type, checked before any device is touched
        edge_type = getattr(data, "edge_type", None)
        if not torch.is_tensor(edge_type) or edge_type.dtype != torch.int64:
            raise ValueError("use_edge_type=True needs data.edge_type: an int64 tensor of shape [E]")
        if edge_type.dim() != 1 or edge_type.numel() != data.edge_index.size(1):
            raise ValueError(f"data.edge_type must have shape [E] = [{data.edge_index.size(1)}], got "
                             f"{tuple(edge_type.shape)}")

    # ---- device (reference :246-258): the message-passing path is HIP-only -------------------
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if distributed is None:  # one of several ranks a launcher started, and a model with a node-partitioned form
        from .dist.experiment import SUPPORTED
        distributed = world > 1 and name in SUPPORTED and not post_cs and model is None
    dist_ctx = None
    if distributed and num_neighbors is not None:
        raise NotImplementedError("num_neighbors is not implemented on the partitioned (distributed) route")
    if distributed and use_edge_weight:
        raise NotImplementedError("use_edge_weight=True is not implemented on the partitioned (distributed) route")
    if distributed and use_edge_attr:
        raise NotImplementedError("use_edge_attr=True is not implemented on the partitioned (distributed) route")
    if distributed and use_edge_type:
        raise NotImplementedError("use_edge_type=True is not implemented on the partitioned (distributed) route")
    if distributed and model is None and (model_init_param or {}).get("aggr", "mean") != "mean":
        raise NotImplementedError(f"aggr={model_init_param['aggr']!r} is not implemented on the partitioned (distributed) "
                                  "route: its exchange carries sums")
    if distributed:
        from .dist.experiment import DistContext
        dist_ctx = DistContext.open(name, post_cs, use_cpu)  # process group, rank's device; raises for unsupported set-ups
        cuda_index = dist_ctx.cuda_index
    elif model is None and name != "mlp" and (use_cpu or not torch.cuda.is_available()):
        raise RuntimeError("rgb_experiment_amd runs message passing in HIP kernels on an MI355X device; "
                           "use_cpu=True / no visible GPU is not supported (no CPU fallback)")
    device = dist_ctx.device if dist_ctx is not None else torch.device(
        f"cuda:{cuda_index}" if (torch.cuda.is_available() and not use_cpu) else "cpu")
    data = data.to(device)
    if to_undirected_graph:  # reference :235-238 (there on the CPU, before .to(device)); here on the run's device: the
        data.edge_index = to_undirected(data.edge_index, num_nodes=data.num_nodes)  # HIP radix sort + unique on a GPU
    edge_weight = None
    if use_edge_weight:
        edge_weight = getattr(data, "edge_weight", None)
        if not torch.is_tensor(edge_weight) or not edge_weight.is_floating_point():
            raise ValueError("use_edge_weight=True needs data.edge_weight: a float tensor of shape [E]")
        if edge_weight.dim() != 1 or edge_weight.numel() != data.edge_index.size(1):
            raise ValueError(f"data.edge_weight must have shape [E] = [{data.edge_index.size(1)}], got "
                             f"{tuple(edge_weight.shape)}")
        edge_weight = edge_weight.detach().to(torch.float32).contiguous()
    edge_attr = None
    if use_edge_attr:
        edge_attr = data.edge_attr.detach().to(torch.float32).contiguous()
    edge_type = data.edge_type.detach().contiguous() if use_edge_type else None
    features = data.x
    if normalize_feature in ("row", "col", "all"):
        features = _normalize_features(features, normalize_feature, normalize_feature_method)
    if dist_ctx is None and features.is_cuda:
        # F = 1433 (Cora) rows start on 4-byte boundaries only: kept at a row stride of 1436 floats every dense product over
        # the features (x W^T forward, dW = dY^T x backward) reads them with 16-byte loads; bag-of-words features (Cora:
        # 1.3 % non-zeros) are multiplied over their non-zeros alone (ops.prepare_features: same values, same sums)
        from . import ops
        features = ops.prepare_features(features)

    if need_to_reappear:  # reference :305-310
        random.seed(reappear_seed)
        np.random.seed(reappear_seed)
        torch.manual_seed(reappear_seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed(reappear_seed)

    # ---- model (reference :315-391) ----------------------------------------------------------
    input_dim = data.num_node_features
    output_dim = int(data.y.max().item()) + 1
    y = data.y
    train_mask, val_mask, test_mask = (_as_bool_mask(m, data.num_nodes, device)
                                       for m in (data.train_mask, data.val_mask, data.test_mask))
    # the reference's NLLLoss(out[mask], y[mask]) (:400,429) raises on a label outside [0, C); the masked loss kernels
    # would skip such a row instead (different row set, different mean): refuse here, once, on the host
    for part, m in (("train", train_mask), ("val", val_mask), ("test", test_mask)):
        sel = y[m]
        if sel.numel() and (int(sel.min()) < 0 or int(sel.max()) >= output_dim):
            raise RuntimeError(f"{part}_mask selects nodes whose label is outside [0, {output_dim}) "
                               "(e.g. -1 = unlabelled): the reference's NLLLoss would raise on them")
    is_pta = name == "pta" and model is None
    if model is not None:  # the caller's module: `model_name` is a label only, `model_init_param` is not read
        if not isinstance(model, nn.Module):
            raise TypeError(f"model must be a torch.nn.Module, got {type(model).__name__}")
        net = model
        params = inspect.signature(net.forward).parameters
        takes_edges = "edge_index" in params or any(p.kind is p.VAR_KEYWORD for p in params.values())
        fwd = {"x": features, "edge_index": data.edge_index} if takes_edges else {"x": features}
        if edge_attr is not None:
            fwd["edge_attr"] = edge_attr
        if edge_type is not None:
            fwd["edge_type"] = edge_type
    elif is_pta:  # reference :351-374
        adj = normalized_adjacency(data.edge_index, data.num_nodes)
        idx = [m.nonzero(as_tuple=True)[0] for m in (train_mask, val_mask, test_mask)]
        K, alpha = model_init_param["K"], model_init_param["alpha"]
        y_soft = [label_propagation(adj, y, i, K, alpha) for i in idx]
        net = MODELS[name](nfeat=input_dim, nclass=output_dim, **model_init_param)
        fwd = {"x": features}
    else:
        net = MODELS[name](input_dim=input_dim, output_dim=output_dim, **model_init_param)
        fwd = {"x": features} if name == "mlp" else {"x": features, "edge_index": data.edge_index}
        if edge_weight is not None:
            fwd["edge_weight"] = edge_weight
        if edge_attr is not None:
            fwd["edge_attr"] = edge_attr
        if edge_type is not None:
            fwd["edge_type"] = edge_type
    net.to(device)
    uses_graph = name != "mlp" if model is None else "edge_index" in fwd
    if model is not None:  # one eval-mode forward before the loop: the contract of the returned mapping
        net.eval()
        with torch.no_grad():
            probe = net(**fwd)
        if not (hasattr(probe, "__getitem__") and hasattr(probe, "__contains__") and "emb" in probe and "out" in probe):
            raise ValueError("experiment(model=...): the module's forward must return a mapping with 'out' (log-"
                             "probabilities) and 'emb' (logits), as the models of this package do")
        del probe
    sampler = None
    if num_neighbors is not None:
        # neighbour-sampled training: shapes change per batch (no capture), and a kept whole-graph aggregate must never
        # reach a batch forward
        from .sampler import NeighborSampler
        sampler = NeighborSampler(data.edge_index, data.num_nodes, num_neighbors)
        train_rows = train_mask.nonzero(as_tuple=True)[0]
        cache_input_aggregate = False
        use_hip_graph = False
    if cache_input_aggregate == "auto":  # memory guard: the kept aggregate is one more [N, F] fp32 matrix in HBM
        cache_input_aggregate = (device.type == "cuda" and name != "mlp" and dist_ctx is None  # partitioned: opt-in only
                                 and model is None
                                 and features.numel() * 4 <= torch.cuda.mem_get_info(device)[0] // 4)
    if cache_input_aggregate:
        net.cache_input_aggregate = True  # read by models/_stack.ConvStack; other models have no such form
    runner = None
    if dist_ctx is not None:
        # 1-D node partition: this rank keeps its node range of features / labels / masks and the structures of its
        # share of the graph; parameters are replicated (the seeds above made them equal on every rank)
        runner = dist_ctx.runner(net, data.edge_index, features, y, (train_mask, val_mask, test_mask), learning_rate,
                                 weight_decay, cache_input_aggregate, task_split, share_eval_forward)
        use_hip_graph = False
    graphed = None
    # capturable Adam keeps its step count on the device: required for graph capture, and used for the
    # eager GPU loop too so that both loops run the very same update kernels
    optimizer = torch.optim.Adam(net.parameters(), lr=learning_rate, weight_decay=weight_decay,
                                 capturable=device.type == "cuda")
    want_graph = bool(use_hip_graph) and device.type == "cuda" and not is_pta
    is_supergat = name == "supergat" and model is None
    if want_graph and is_supergat:
        say("SuperGAT draws its edge samples every step: running the eager loop (use_hip_graph is ignored)")
        want_graph = False
    if want_graph and use_hip_graph != "always" and uses_graph and data.edge_index.size(1) > HIP_GRAPH_MAX_EDGES:
        say(f"{data.edge_index.size(1)} edges: the epoch is kernel-bound, running the eager loop (use_hip_graph='always' "
            "forces the capture)")
        want_graph = False
    if want_graph:
        from .epoch_graph import GraphedEpoch
        try:
            graphed = GraphedEpoch(net, optimizer, fwd, y, (train_mask, val_mask, test_mask),
                                   share_eval_forward).capture()
        except Exception as exc:  # stay on the (GPU) eager loop; never a CPU path
            say(f"hipGraph capture failed ({exc!r}); running the eager loop")
            torch.cuda.synchronize()
            graphed = None
            optimizer = torch.optim.Adam(net.parameters(), lr=learning_rate, weight_decay=weight_decay,
                                         capturable=True)
    criterion = nn.NLLLoss()

    hist = {k: [] for k in ("train_acc", "train_loss", "val_acc", "val_loss", "test_acc", "test_loss")}
    best_state, best_val_loss, best_val_acc, patience = {}, 0, 0, 0
    best_pta_metrics = None

    # Inside the loop the reference computes sklearn precision/recall/F1 on the CPU for train, val and
    # test every epoch (:434,:464,:470) and then uses only 'ACC' of each; the returned dict comes from
    # the final test() (:512). Accuracy alone is therefore computed in the loop (no host copies of the
    # prediction vectors), the full metrics once at the end: same return values, fewer syncs.
    loop_metrics = False

    def sampled_epoch():
        """An epoch on neighbour-sampled mini-batches (num_neighbors). Training: permute the training rows, cut them into
        batches of batch_size seeds, and per batch sample, gather features and labels, run the training forward on the
        batch's (x, edge_index), take the masked cross-entropy on the seed rows, backward, one optimizer step. Then the
        full-graph eval forwards, as generic_epoch takes them on the GPU."""
        from . import ops
        from .graph import forget
        from .models._stack import masked_ce, masked_ce_pair
        net.train()
        order = train_rows[torch.randperm(train_rows.numel(), device=device)]
        sums = torch.zeros(3, dtype=torch.float64, device=device)  # loss * seeds, seeds, correct
        for b0 in range(0, order.numel(), batch_size):
            # (a slice of a permutation of in-range rows: distinct and in range by construction, no check and no read-back)
            batch = sampler.sample_unchecked(order[b0:b0 + batch_size])
            x_b = ops.gather_rows(features, batch.n_id.to(torch.int32))
            y_b = y[batch.n_id]
            seed_rows = torch.arange(batch.n_id.numel(), device=device) < batch.num_seeds
            fwd_b = dict(fwd, x=x_b)
            if "edge_index" in fwd_b:
                fwd_b["edge_index"] = batch.edge_index
            optimizer.zero_grad()
            loss, stats = masked_ce(net, fwd_b, y_b, seed_rows)
            if is_supergat:  # reference :431-432
                loss = loss + supergat_graph_lambda * net.att_loss
            loss.backward()
            optimizer.step()
            forget(batch.edge_index)  # the batch's CSRs are not met again: keep the whole graph's in the cache
            sums += torch.stack([loss.detach().double() * stats[1], stats[1], stats[2]])
        total_loss, seeds, hits = sums.tolist()  # the training side's one read-back of the epoch
        hist["train_loss"].append(total_loss / seeds if seeds else float("nan"))
        hist["train_acc"].append(hits / seeds if seeds else float("nan"))
        net.eval()
        with torch.no_grad():
            if share_eval_forward:
                st = masked_ce_pair(net, fwd, y, val_mask, test_mask)
            else:
                st = torch.stack([masked_ce(net, fwd, y, val_mask)[1], masked_ce(net, fwd, y, test_mask)[1]])
        (vn, vc, vh), (sn, sc, sh) = st.tolist()
        nan = float("nan")
        hist["test_acc"].append(sh / sc if sc else nan)
        hist["test_loss"].append(sn / sc if sc else nan)
        return (vh / vc if vc else nan), (vn / vc if vc else nan), None

    def generic_epoch(i):
        """reference :427-440, :464-473: 1 train forward+backward, 2 eval forwards."""
        if runner is not None:  # the same epoch on the node partition; the five numbers are all-reduced over the ranks
            # more=True: the next epoch's training forward + backward may be computed during this epoch's eval forwards
            # (its optimizer step waits for the next call; the model is untouched until then, see DistRunner.epoch)
            tl, vl, va, sl, sa = runner.epoch(more=i < epoch - 1)
            for key, v in (("train_loss", tl), ("train_acc", float("nan")), ("test_loss", sl), ("test_acc", sa)):
                hist[key].append(v)
            return va, vl, None
        if graphed is not None:
            tl, ta, vl, va, sl, sa = graphed.run()
            hist["train_loss"].append(tl)
            hist["train_acc"].append(ta)
            hist["test_loss"].append(sl)
            hist["test_acc"].append(sa)
            return va, vl, None
        if sampler is not None:
            return sampled_epoch()
        net.train()
        optimizer.zero_grad()
        if device.type == "cuda":
            # NLLLoss on out[train_mask] (reference :429) and the train accuracy (:434) of the training forward — the
            # same kernels as the captured epoch (models/_stack.masked_ce), so both loops train bit-identically
            from .models._stack import masked_ce
            loss, stats = masked_ce(net, fwd, y, train_mask)
            if is_supergat:  # reference :431-432
                loss = loss + supergat_graph_lambda * net.att_loss
            hist["train_acc"].append((stats[2] / stats[1]).item())
        else:
            res = net(**fwd)
            out = res["out"]
            loss = criterion(out[train_mask], y[train_mask])
            hist["train_acc"].append(compare_pred_label(out[train_mask].max(dim=1)[1], y[train_mask],
                                                        loop_metrics)["ACC"])
        hist["train_loss"].append(loss.item())
        loss.backward()
        optimizer.step()
        if device.type == "cuda":
            # the eval forwards reduced to what the loop reads of them (loss and accuracy per mask), by the same kernels
            # as the captured epoch: NLL sum / rows / arg-max hits from the last conv's kernel where the model has that
            # form, else from its logits; one forward for both masks under share_eval_forward
            from .models._stack import masked_ce, masked_ce_pair
            net.eval()
            with torch.no_grad():
                if share_eval_forward:
                    st = masked_ce_pair(net, fwd, y, val_mask, test_mask)
                else:
                    st = torch.stack([masked_ce(net, fwd, y, val_mask)[1], masked_ce(net, fwd, y, test_mask)[1]])
            (vn, vc, vh), (sn, sc, sh) = st.tolist()  # the epoch's one read-back of the eval side
            nan = float("nan")
            hist["test_acc"].append(sh / sc if sc else nan)
            hist["test_loss"].append(sn / sc if sc else nan)
            return (vh / vc if vc else nan), (vn / vc if vc else nan), None
        val = test(net, fwd, y, val_mask, loop_metrics)
        val_loss = criterion(val["test_op"][val_mask], y[val_mask]).item()
        if share_eval_forward:  # same eval-mode outputs, second mask (opt-in: the reference forwards twice)
            tst = {"test_op": val["test_op"],
                   "ACC": compare_pred_label(val["test_op"][test_mask].max(dim=1)[1], y[test_mask],
                                             loop_metrics)["ACC"]}
        else:
            tst = test(net, fwd, y, test_mask, loop_metrics)
        hist["test_acc"].append(tst["ACC"])
        hist["test_loss"].append(criterion(tst["test_op"][test_mask], y[test_mask]).item())
        return val["ACC"], val_loss, None

    def pta_epoch(i):
        """reference :422-425, :442-462 (including its quirk: the test loss is taken on the propagated
        probabilities, not on the logits)."""
        net.train()
        optimizer.zero_grad()
        output = net(features)
        loss = pta_loss_decay * net.loss_function(y_hat=output, y_soft=y_soft[0], epoch=i) \
            + pta_weight_decay * torch.sum(net.Linear1.weight ** 2) / 2
        hist["train_loss"].append(loss.item())
        loss.backward()
        optimizer.step()
        with torch.no_grad():
            prob = net.inference(output.detach(), adj)
            hist["train_acc"].append(compare_pred_label(prob[idx[0]].max(dim=1)[1], y[idx[0]], loop_metrics)["ACC"])
            net.eval()
            output = net(features)
            val_loss = (pta_loss_decay * net.loss_function(y_hat=output, y_soft=y_soft[1])).item()
            prob = net.inference(output, adj)
            val_acc = compare_pred_label(prob[idx[1]].max(dim=1)[1], y[idx[1]], loop_metrics)["ACC"]
            hist["test_loss"].append((pta_loss_decay * net.loss_function(y_hat=prob, y_soft=y_soft[2])).item())
            metrics = compare_pred_label(prob[idx[2]].max(dim=1)[1], y[idx[2]], need_all_metrics)
            metrics["emb"] = prob
        hist["test_acc"].append(metrics["ACC"])
        return val_acc, val_loss, metrics

    # ---- full-batch loop with early stopping (reference :417-504) -------------------------------
    for i in range(epoch):
        val_acc, val_loss, pta_metrics = (pta_epoch if is_pta else generic_epoch)(i)
        hist["val_acc"].append(val_acc)
        hist["val_loss"].append(val_loss)
        if i == 0:
            best_val_loss, best_val_acc = val_loss, val_acc
        if early_stopping_criterion == "loss":
            improved = val_loss <= best_val_loss
        elif early_stopping_criterion == "acc":
            improved = val_acc >= best_val_acc
        else:
            raise ValueError(f"early_stopping_criterion {early_stopping_criterion!r} not in loss/acc")
        if improved:
            patience = 0
            best_val_loss, best_val_acc = min(val_loss, best_val_loss), max(val_acc, best_val_acc)
            best_state = deepcopy(net.state_dict())
            best_pta_metrics = pta_metrics
        elif implement_early_stopping and i > begin_early_stopping:
            patience += 1
            if patience > early_stopping:
                break

    if runner is not None:
        runner.discard_speculation()  # the loop stopped early: a step computed ahead is dropped
    if best_state:
        net.load_state_dict(best_state)
    if is_pta:  # reference :509-510
        final = dict(best_pta_metrics)
        final.setdefault("label", y[idx[2]])
        final.setdefault("pred", final["emb"][idx[2]].max(dim=1)[1])
    elif runner is not None:  # every rank's test rows gathered: the same metrics dict on every rank
        final = dist_ctx.final_test(runner, y, test_mask, need_all_metrics, compare_pred_label)
    else:
        final = test(net, fwd, y, test_mask, need_all_metrics)

    if post_cs:  # reference :516-534: C&S on exp(log-probs) of the best model, metrics on the test rows
        from .nn import CorrectAndSmooth
        if data.edge_index.device.type != "cuda":
            raise RuntimeError("post_cs runs its propagation in HIP kernels; a GPU is required (no CPU fallback)")
        post = CorrectAndSmooth(**(cs_param or InitialParameters.default_cs_param))
        y_soft = final["test_op"].exp()
        cs_weight = {} if edge_weight is None else {"edge_weight": edge_weight}
        y_soft = post.correct(y_soft, y[train_mask], train_mask, data.edge_index, **cs_weight)
        y_soft = post.smooth(y_soft, y[train_mask], train_mask, data.edge_index, **cs_weight)
        pred = y_soft.max(dim=1)[1][test_mask]
        cs = compare_pred_label(pred, y[test_mask], need_all_metrics)
        final.update(cs)
        final["pred"], final["label"] = pred, y[test_mask]

    if print_confusion_matrix:
        k = output_dim
        cm = torch.zeros(k, k, dtype=torch.long)
        for t, p in zip(final["label"].cpu().tolist(), final["pred"].cpu().tolist()):
            cm[t, p] += 1
        print(cm.numpy())
    if check_data_valid:  # reference :575-584
        print("train/val/test sizes:", int(train_mask.sum()), int(val_mask.sum()), int(test_mask.sum()))
        print("overlaps train&val, train&test, val&test:", int((train_mask & val_mask).sum()),
              int((train_mask & test_mask).sum()), int((val_mask & test_mask).sum()))

    result = {k: final[k] for k in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro")}
    if return_model:
        result["model"] = net
        result["history"] = hist
        result["used_hip_graph"] = graphed is not None
        result["emb"] = final["emb"]
        if runner is not None:
            result["distributed"] = {"world": dist_ctx.world, "rank": dist_ctx.rank, "rows": (runner.lo, runner.hi),
                                     "fused_schedule": runner.engine is not None,
                                     "task_split_role": getattr(runner, "role", None),
                                     "test_rows": int(final["label"].numel())}
    return result
