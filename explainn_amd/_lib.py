"""ctypes binding of libexplainn_hip.so (C ABI: include/explainn_hip.h).

The library is the product; there is no CPU or eager-PyTorch fallback.  `load()` raises if the
shared object is missing (run `python -c "import __graft_entry__ as g; g.build()"` or
`make -C explainn_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EXPLAINN_HIP_LIB", os.path.join(_HERE, "libexplainn_hip.so"))

OK, E_ARG, E_HIP, E_BATCH1, E_STATE, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5
LOSS_BCE_WITH_LOGITS, LOSS_MSE = 0, 1
PWM_SUM, PWM_MAX = 0, 1
METRICS_GLOBAL, METRICS_PER_TASK = 0, 1
METRICS_BINARY, METRICS_LINEAR = 0, 1
METRICS_NONFINITE, METRICS_NOT_BINARY = 1, 2
IG_BASELINE_ZERO, IG_BASELINE_UNIFORM, IG_BASELINE_CODES = 0, 1, 2
SCAN_AUTO, SCAN_WINDOWS, SCAN_SHARED = 0, 1, 2
MOTIF_MAX_WIDTH = 64      # EXPLAINN_MOTIF_MAX_WIDTH: columns per motif of explainn_motif_compare
MOTIF_MAX_BINS = 128      # EXPLAINN_MOTIF_MAX_BINS: score bins per column of explainn_motif_significance
MOTIF_NO_SCORE = 255      # EXPLAINN_MOTIF_NO_SCORE: a colscore entry without a column
LINKAGE_SINGLE, LINKAGE_COMPLETE, LINKAGE_AVERAGE = 0, 1, 2
MOTIF_TREE_MAX_LEAVES = 12288   # EXPLAINN_MOTIF_TREE_MAX_LEAVES: motifs of one explainn_motif_tree call
SITES_TILE = 1024        # EXPLAINN_SITES_TILE: start positions per workgroup of explainn_call_sites
PWM_GROUP = 16           # EXPLAINN_PWM_GROUP: motifs per workgroup of explainn_pwm_sites
PWM_HIST_SLICE = 1 << 30  # EXPLAINN_PWM_HIST_SLICE: starts per workgroup of explainn_pwm_score_histogram at the most
SITEQ_MAX_BINS = 32768   # EXPLAINN_SITEQ_MAX_BINS: score bins per unit of explainn_site_qvalues
ACT_BINS = 32768         # EXPLAINN_ACT_BINS: one bin per non-negative float16 bit pattern
ACT_SPAN = 8192          # EXPLAINN_ACT_SPAN: start positions a workgroup of explainn_activation_histogram takes at a time
BEST_SPAN = 256          # EXPLAINN_BEST_SPAN: starts a wavefront of explainn_record_best takes per pass over its record
PWM_BEST_SPAN = 256      # EXPLAINN_PWM_BEST_SPAN: the same of explainn_pwm_record_best
PWM_VARIANT_MAX_ALLELE = 128  # EXPLAINN_PWM_VARIANT_MAX_ALLELE: bases per allele of explainn_pwm_variant_best
WORD_MIN_WIDTH, WORD_MAX_WIDTH = 3, 10   # EXPLAINN_WORD_MIN_WIDTH, EXPLAINN_WORD_MAX_WIDTH: the k of the word entry points
WORD_SPAN = 256          # EXPLAINN_WORD_SPAN: starts a workgroup of the word kernels takes per pass over its record
SPACING_MAX_DISTANCE = 1024  # EXPLAINN_SPACING_MAX_DISTANCE: the largest max_distance of explainn_site_spacing
CENTRALITY_MAX_THRESHOLDS = 16      # EXPLAINN_CENTRALITY_MAX_THRESHOLDS: thresholds of one explainn_site_positions call
CENTRALITY_MAX_REGIONS = 4194304    # EXPLAINN_CENTRALITY_MAX_REGIONS: regions per unit of explainn_centrality_test

_fp = C.c_void_p          # device pointers travel as integers (tensor.data_ptr())

PARAM_FIELDS = (
    "conv_w", "conv_b", "bn1_w", "bn1_b", "bn1_rm", "bn1_rv",
    "fc1_w", "fc1_b", "bn2_w", "bn2_b", "bn2_rm", "bn2_rv",
    "fc2_w", "fc2_b", "bn3_w", "bn3_b", "bn3_rm", "bn3_rv",
    "final_w", "final_b", "bn1_nbt", "bn2_nbt", "bn3_nbt",
)
# C field -> reference state_dict key (architectures/__init__.py:72-104)
PARAM_KEYS = {
    "conv_w": "linears.0.weight", "conv_b": "linears.0.bias",
    "bn1_w": "linears.1.weight", "bn1_b": "linears.1.bias",
    "bn1_rm": "linears.1.running_mean", "bn1_rv": "linears.1.running_var",
    "fc1_w": "linears.6.weight", "fc1_b": "linears.6.bias",
    "bn2_w": "linears.7.weight", "bn2_b": "linears.7.bias",
    "bn2_rm": "linears.7.running_mean", "bn2_rv": "linears.7.running_var",
    "fc2_w": "linears.10.weight", "fc2_b": "linears.10.bias",
    "bn3_w": "linears.11.weight", "bn3_b": "linears.11.bias",
    "bn3_rm": "linears.11.running_mean", "bn3_rv": "linears.11.running_var",
    "final_w": "final.weight", "final_b": "final.bias",
    "bn1_nbt": "linears.1.num_batches_tracked", "bn2_nbt": "linears.7.num_batches_tracked",
    "bn3_nbt": "linears.11.num_batches_tracked",
}
GRAD_FIELDS = ("conv_w", "conv_b", "bn1_w", "bn1_b", "fc1_w", "fc1_b", "bn2_w", "bn2_b",
               "fc2_w", "fc2_b", "bn3_w", "bn3_b", "final_w", "final_b")

SYNC_PHASES = 8
SYNC_ARG_FIELDS = ("x", "targets", "dlogits", "dl_scale", "B_local", "B_global", "params", "grads",
                   "loss_kind", "dropout_p", "seed", "keep_mask", "freeze_top_n_filters", "logits",
                   "loss_out")


class Params(C.Structure):
    _fields_ = [(f, _fp) for f in PARAM_FIELDS] + [("version", C.c_uint64)]


class Grads(C.Structure):
    _fields_ = [(f, _fp) for f in GRAD_FIELDS]


class ExplainnError(RuntimeError):
    pass


_lib = None


class SyncArgs(C.Structure):
    """explainn_sync_args: one sync-BN step's arguments (include/explainn_hip.h)."""
    _fields_ = [("x", _fp), ("targets", _fp), ("dlogits", _fp), ("dl_scale", C.c_float),
                ("B_local", C.c_int), ("B_global", C.c_int), ("params", C.POINTER(Params)),
                ("grads", C.POINTER(Grads)), ("loss_kind", C.c_int), ("dropout_p", C.c_float),
                ("seed", C.c_uint64), ("keep_mask", _fp), ("freeze_top_n_filters", C.c_int),
                ("logits", _fp), ("loss_out", _fp)]


EDIT_FIELDS = ("row_start", "row_edit", "pos", "ref_len", "alt_len", "alt_off", "alt", "n_edits", "alt_bytes")


class Edits(C.Structure):
    """explainn_edits: the row table, the edit table and the alt pool of explainn_score_edits (device
    pointers; include/explainn_hip.h)."""
    _fields_ = [(f, _fp) for f in EDIT_FIELDS[:7]] + [(f, C.c_int64) for f in EDIT_FIELDS[7:]]


HAPLOTYPE_FIELDS = ("row_start", "row_first", "row_count", "edit_index", "pos", "ref_len", "alt_len", "alt_off",
                    "alt", "n_index", "n_edits", "alt_bytes")


class Haplotypes(C.Structure):
    """explainn_haplotypes: the row table, the index lists, the edit table and the alt pool of
    explainn_score_haplotypes (device pointers; include/explainn_hip.h)."""
    _fields_ = [(f, _fp) for f in HAPLOTYPE_FIELDS[:9]] + [(f, C.c_int64) for f in HAPLOTYPE_FIELDS[9:]]


_ctx, _pp, _gp, _i, _i64 = C.c_void_p, C.POINTER(Params), C.POINTER(Grads), C.c_int, C.c_int64
# every C function of the header: name -> (restype, argtypes)
SIGNATURES = {
    "explainn_create": (_i, [C.POINTER(_ctx), _i, _i, _i, _i, _i, _i]),
    "explainn_create_bank": (_i, [C.POINTER(_ctx), _i, _i, _i, _i, _i, _i, _i]),
    "explainn_groups": (_i, [_ctx]),
    "explainn_destroy": (None, [_ctx]),
    "explainn_last_error": (C.c_char_p, []),
    "explainn_scratch_bytes": (_i64, [_ctx]),
    "explainn_forward_eval": (_i, [_ctx, _fp, _i, _pp, _fp, _fp]),
    "explainn_forward_train": (_i, [_ctx, _fp, _i, _pp, _fp, C.c_float, C.c_uint64, _fp, _fp]),
    "explainn_backward": (_i, [_ctx, _fp, _i, _pp, _gp, _i, _fp]),
    "explainn_forward_eval_keep": (_i, [_ctx, _fp, _i, _pp, _fp, _fp]),
    "explainn_input_grad": (_i, [_ctx, _fp, _i, _pp, _fp, _fp]),
    "explainn_backward_input": (_i, [_ctx, _fp, _i, _pp, _gp, _i, _fp, _fp]),
    "explainn_ism_workspace_bytes": (_i64, [_ctx, _i]),
    "explainn_ism": (_i, [_ctx, _fp, _i, _pp, _fp, _fp, _fp, _i64, _fp]),
    "explainn_evolve_pick": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, C.c_float, _fp, _fp, _fp, _fp, _fp]),
    "explainn_integrated_gradients_workspace_bytes": (_i64, [_ctx, _i]),
    "explainn_integrated_gradients": (_i, [_ctx, _fp, _i, _pp, _i, _fp, _fp, _i, _fp, _fp, _fp, _fp, _i64, _fp]),
    "explainn_loss_grad": (_i, [_ctx, _i, _fp, _fp, _i, _fp, _fp, _fp]),
    "explainn_train_step": (_i, [_ctx, _fp, _fp, _i, _pp, _gp, _i, C.c_float, C.c_uint64, _i, _fp, _fp,
                                 _fp]),
    "explainn_train_step_fc": (_i, [_ctx, _fp, _fp, _i, _pp, _gp, _i, C.c_float, C.c_uint64, _fp, _fp,
                                    _fp]),
    "explainn_train_step_conv": (_i, [_ctx, _i, _pp, _gp, _i, _fp]),
    "explainn_unit_outputs": (_i, [_ctx, _fp, _i, _pp, _fp, _fp]),
    "explainn_unit_activations": (_i, [_ctx, _fp, _i, _pp, _fp, _fp]),
    "explainn_filter_act_max": (_i, [_ctx, _fp, _i, _pp, _fp, _fp, _fp]),
    "explainn_filter_sites": (_i, [_ctx, _fp, _i, _pp, _fp, _fp, _i, _fp, _fp, _fp, _fp]),
    "explainn_stage_codes": (_i, [_ctx, _fp, _i, _i, _fp]),
    "explainn_stage_onehot": (_i, [_ctx, _fp, _i, _fp]),
    "explainn_stage_windows": (_i, [_ctx, _fp, _i64, _i64, _i64, _i, _i, _fp]),
    "explainn_scan_workspace_bytes": (_i64, [_ctx, _i64, _i64, _i]),
    "explainn_scan": (_i, [_ctx, _fp, _i64, _i64, _i64, _i64, _i, _pp, _fp, _i, _fp, _i64, _fp]),
    "explainn_stage_edited_windows": (_i, [_ctx, _fp, _i64, C.POINTER(Edits), _i64, _i, _i, _fp]),
    "explainn_score_edits": (_i, [_ctx, _fp, _i64, C.POINTER(Edits), _i64, _i, _pp, _fp, _fp, _fp]),
    "explainn_stage_haplotype_windows": (_i, [_ctx, _fp, _i64, C.POINTER(Haplotypes), _i64, _i, _i, _fp]),
    "explainn_score_haplotypes": (_i, [_ctx, _fp, _i64, C.POINTER(Haplotypes), _i64, _i, _pp, _fp, _fp, _fp]),
    "explainn_call_sites_workspace_bytes": (_i64, [_ctx, _i64]),
    "explainn_call_sites": (_i, [_ctx, _fp, _i64, _i64, _i64, _i64, _i, _pp, _fp, _fp, _fp, _fp, _i64, _fp,
                                 _i64, _fp]),
    "explainn_activation_histogram": (_i, [_ctx, _fp, _i64, _i64, _i64, _i64, _i, _pp, _fp, _fp]),
    "explainn_activation_null": (_i, [_fp, _i, C.c_double, _fp, _fp, _fp, _fp]),
    "explainn_site_spacing": (_i, [_fp, _fp, _i, _fp, _i, _fp, _i, _i, _fp, _fp]),
    "explainn_spacing_test": (_i, [_fp, _i, _i, _fp, _fp, _i, _i, _i64, _fp, _fp, _fp, _fp, _fp]),
    "explainn_record_best": (_i, [_ctx, _fp, _i64, _fp, _i64, _i, _pp, _fp, _fp, _fp]),
    "explainn_enrichment_workspace_bytes": (_i64, [_i, _i64]),
    "explainn_enrichment_test": (_i, [_fp, _fp, _i, _i64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                      _i64, _fp]),
    "explainn_site_positions": (_i, [_fp, _fp, _fp, _fp, _i, _i64, _i, _i, _fp, _fp, _fp]),
    "explainn_centrality_test": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _i, _i64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                      _fp, _fp, _fp, _fp]),
    "explainn_dense_input": (_i, [_ctx, _i]),
    "explainn_pwm_scan": (_i, [_fp, _i, _i, _fp, _i, _i, _i, _fp, _fp]),
    "explainn_dinucleotide_shuffle": (_i, [_fp, _i64, _i, _i, C.c_uint64, _i64, _i, _fp, _fp, _fp]),
    "explainn_motif_compare_workspace_bytes": (_i64, [_i, _i, _i]),
    "explainn_motif_compare": (_i, [_fp, _fp, _i, _fp, _fp, _i, _i, C.c_float, _i, _i, _fp, _fp, _fp, _fp, _i64,
                                    _fp]),
    "explainn_motif_significance_workspace_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "explainn_motif_significance": (_i, [_fp, _fp, _i, _fp, _fp, _i, _i, C.c_float, _i, _i, _i, _fp, _fp, _fp, _fp,
                                         _fp, _fp, _i64, _fp]),
    "explainn_motif_tree_workspace_bytes": (_i64, [_i, _i]),
    "explainn_motif_tree": (_i, [_fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _i64, _fp]),
    "explainn_motif_tree_cut": (_i, [_fp, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp]),
    "explainn_motif_tree_pool": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp, _fp, _fp]),
    "explainn_pwm_null": (_i, [_fp, _fp, _i, _i, _i, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _fp,
                               _fp, _fp]),
    "explainn_pwm_sites_workspace_bytes": (_i64, [_i, _i64]),
    "explainn_pwm_sites": (_i, [_fp, _i64, _i64, _i64, _i64, _i, _fp, _fp, _i, _i, _fp, _fp, _i, _fp, _fp, _fp, _fp,
                                _i64, _fp, _i64, _fp]),
    "explainn_pwm_score_histogram": (_i, [_fp, _i64, _i64, _i64, _i64, _i, _fp, _fp, _i, _i, _i, _fp, _fp]),
    "explainn_site_qvalues": (_i, [_fp, _fp, _i, _i, C.c_double, _fp, _fp, _fp, _fp]),
    "explainn_pwm_record_best": (_i, [_fp, _i64, _fp, _i64, _i, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp]),
    "explainn_pwm_variant_best": (_i, [_fp, _i64, _fp, _fp, _fp, _fp, _fp, _i64, _i64, _i, _fp, _fp, _i, _i, _fp, _fp,
                                       _fp, _fp]),
    "explainn_word_counts": (_i, [_fp, _i64, _fp, _i64, _i, _i, _fp, _fp, _fp]),
    "explainn_word_test": (_i, [_fp, _fp, _i64, _i64, _i64, _i64, _fp, _fp, _fp, _fp]),
    "explainn_word_sites": (_i, [_fp, _i64, _fp, _i64, _i, _i, _i64, C.c_uint64, _fp, _fp, _fp, _fp, _fp]),
    "explainn_adam_step": (_i, [_i, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp),
                                C.POINTER(_i64), _i64, C.c_double, C.c_double, C.c_double, C.c_double,
                                _fp]),
    "explainn_input_flags": (_i, [_ctx, C.POINTER(_i), _fp]),
    "explainn_stage_timing": (_i, [_ctx, _i]),
    "explainn_stage_count": (_i, []),
    "explainn_stage_name": (C.c_char_p, [_i]),
    "explainn_stage_times": (_i, [_ctx, C.POINTER(C.c_float), _i]),
    "explainn_debug_keep_bits": (_i, [_ctx, _i, _fp, _fp]),
    "explainn_sync_exchange_elems": (_i64, [_ctx, _i]),
    "explainn_sync_phase": (_i, [_ctx, _i, C.POINTER(SyncArgs), _fp, _fp, _fp]),
    "explainn_metrics_workspace_bytes": (_i64, [_i64, _i, _i, _i]),
    "explainn_metrics_binary": (_i, [_fp, _fp, _i64, _i, _i, _fp, _fp, _fp, _fp, _fp, _i64, _fp]),
    "explainn_metrics_linear": (_i, [_fp, _fp, _i64, _i, _i, _fp, _fp, _fp, _fp, _i64, _fp]),
}
EXPORTS = tuple(SIGNATURES)


def load():
    """Load the shared library once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExplainnError(
            "libexplainn_hip.so is not built (%s). explainn_amd has no CPU fallback: build it "
            "with `make -C explainn_amd/csrc` (hipcc, gfx950)." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc):
    """Map a C return code to the exception the reference path would raise."""
    if rc == OK:
        return
    msg = load().explainn_last_error().decode("utf-8", "replace")
    if rc == E_BATCH1:
        # torch.nn.BatchNorm1d raises ValueError for a single value per channel in train mode
        raise ValueError(msg)
    raise ExplainnError("libexplainn_hip: %s (code %d)" % (msg, rc))


# ---------------------------------------------------------------- the call path (context-bound: Context.call)
def device_for(device, candidates, what):
    """The device of a call: the one asked for, else that of the first HIP tensor among `candidates` (looking
    one level into tuples and lists), else the current one.  There is no CPU path: anything else raises, before
    the library is loaded."""
    import torch
    if device is None:
        for obj in candidates:
            first = obj[0] if isinstance(obj, (tuple, list)) and len(obj) else obj
            if torch.is_tensor(first) and first.device.type == "cuda":
                device = first.device
                break
    if device is None and torch.cuda.is_available():
        device = "cuda"
    device = None if device is None else torch.device(device)
    if device is None or device.type != "cuda":
        raise RuntimeError("%s runs only on a HIP device (there is no CPU fallback)" % what)
    if device.index is None and torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def require(t, dtype, shape, device, name):
    """The precondition of a tensor argument: contiguous, of `dtype` and `shape` (None: any size), on `device`
    (None: any HIP device)."""
    import torch
    if not (torch.is_tensor(t) and t.device.type == "cuda" and device in (None, t.device) and t.dtype == dtype and
            t.dim() == len(shape) and all(want in (None, have) for have, want in zip(t.shape, shape)) and
            t.is_contiguous()):
        raise RuntimeError("%s must be a contiguous %s tensor of shape (%s) on %s (there is no CPU fallback)" % (
            name, str(dtype).replace("torch.", ""), ", ".join("*" if n is None else str(n) for n in shape),
            "a HIP device" if device is None else device))
    return t


def arguments(name, device, args):
    """The arguments of the C function `name` as ctypes takes them: a tensor goes as its address (it must be
    contiguous and on `device`, a torch.device with an index), None as NULL, anything else as it is -- numbers,
    ctypes values, byref()s, addresses, and a Structure instance, which ctypes passes by reference where the
    signature says POINTER.  Nothing is loaded or enqueued here."""
    import torch
    argv = list(args)
    for i, a in enumerate(argv):
        if isinstance(a, torch.Tensor):
            if a.device != device or not a.is_contiguous():
                raise RuntimeError("%s: argument %d must be a contiguous tensor on %s (a %s tensor on %s)" % (
                    name, i, device, "contiguous" if a.is_contiguous() else "strided", a.device))
            argv[i] = a.data_ptr()
    return argv


def current_stream(device):
    """The current stream of `device` as the C functions take it.  The raw handle, as torch's own generated
    launchers read it: torch.cuda.current_stream() builds a Stream object around it at 2 us a call, more than
    the rest of Context.call together."""
    import torch
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(device.index))


def call(name, device, *args):
    """Enqueue the C function `name` on the current stream of `device` with `arguments`; the stream is the last
    argument."""
    import torch
    device = torch.device(device)
    argv = arguments(name, device, args)
    fn = getattr(load(), name)
    with torch.cuda.device(device):
        check(fn(*argv, current_stream(device)))


def workspace(name, device, *dims):
    """(uint8 tensor on `device`, nbytes) for the size export `name` at `dims`; a negative size is the export's
    refusal and raises ValueError with its text."""
    import torch
    lib = load()
    nbytes = int(getattr(lib, name)(*dims))
    if nbytes < 0:
        raise ValueError(lib.explainn_last_error().decode("utf-8", "replace"))
    return torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device), nbytes


class Context:
    """Owner of one explainn_ctx (device scratch for a fixed model geometry and max batch)."""

    def __init__(self, cnn_units, kernel_size, sequence_length, n_features, max_batch, device, groups=1):
        """groups > 1: a model bank of `groups` members of cnn_units units each (explainn_create_bank)."""
        self.lib = load()
        self.geom = (cnn_units, kernel_size, sequence_length, n_features)
        self.groups = groups
        self.max_batch = max_batch
        self.device = device
        h = C.c_void_p()
        if groups == 1:
            check(self.lib.explainn_create(C.byref(h), cnn_units, kernel_size, sequence_length,
                                           n_features, max_batch, device))
        else:
            check(self.lib.explainn_create_bank(C.byref(h), groups, cnn_units, kernel_size,
                                                sequence_length, n_features, max_batch, device))
        self.handle = h
        import torch
        self.torch_device = torch.device("cuda", device)

    def call(self, name, *args):
        """Enqueue the C function `name` of this context on the current stream of its device: the handle, then
        `arguments`, then the stream.  No torch.cuda.device scope is entered: the caller is in one
        (ExplaiNN._launch).  The entry points without a stream argument are called on `lib` directly."""
        argv = arguments(name, self.torch_device, args)
        check(getattr(self.lib, name)(self.handle, *argv, current_stream(self.torch_device)))

    def workspace(self, name, *dims):
        """(uint8 tensor on this context's device, nbytes) for the size export `name`(handle, *dims); a negative
        size is a return code and raises as `check` does."""
        import torch
        nbytes = int(getattr(self.lib, name)(self.handle, *dims))
        check(min(nbytes, 0))
        return torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.torch_device), nbytes

    def stage_timing(self, enable=True):
        check(self.lib.explainn_stage_timing(self.handle, int(bool(enable))))

    def stage_times(self):
        """{stage name: microseconds} of the last training step (device-synchronising)."""
        n = self.lib.explainn_stage_count()
        buf = (C.c_float * n)()
        check(self.lib.explainn_stage_times(self.handle, buf, n))
        return {self.lib.explainn_stage_name(i).decode(): float(buf[i]) for i in range(n) if buf[i] >= 0}

    def scratch_bytes(self):
        return int(self.lib.explainn_scratch_bytes(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.explainn_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
