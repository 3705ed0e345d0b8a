"""The state that outlives a call, what each piece owes to the stream it is used on, and the rows of tests/test_hip_streams.py
(profiles/stream_tests_notes.md §1 repeats RECORDS as a table).  tests/test_stream_cases_cpu.py holds this file to the code: a new
module-level cache of the package, or a new static container of csrc/, without a record here fails it.

A record: owner (where it lives), names (the identifiers it covers), key, init (what initialises it, on which stream), resets (does it put
itself back for the next call), capture (what happens while the stream is capturing), rows (the surfaces of ROWS that exercise it;
empty: a documented contract only, run by history_cases.row_user_stream)."""

LAYER_CONTRACT = "one stream per layer at a time; the caller orders a change of stream"


def _rec(owner, names, key, init, resets, capture, rows=()):
    return dict(owner=owner, names=tuple(names), key=key, init=init, resets=resets, capture=capture, rows=tuple(rows))


RECORDS = [
    # ---- library state (csrc/)
    _rec("csrc/loss_voxel.hip si_scratch", ["si_scratch.bufs"], "(device, raw stream)",
         "hipMalloc, then hipMemsetAsync of the partial sums and the ticket ON the stream that will use it", "the last workgroup puts the ticket back to 0",
         "never handed to a capturing stream: the two-launch form (zero-fill + atomics on `stats`) is recorded", ["si_loss", "si_log_loss"]),
    _rec("csrc/loss_voxel.hip voxel_id_scratch", ["voxel_id_scratch.bufs"], "(device, raw stream)",
         "hipMalloc; never initialised: the sort kernel writes every record and table entry the band kernel reads, on the same stream",
         "nothing to reset; regrown (after hipStreamSynchronize of its stream) when a launch needs more", "never handed to a capturing stream: the atomic / id-less forms are recorded",
         ["voxel_sorted"]),
    _rec("csrc/pointwise.hip allow_full_lds", ["allow_full_lds.done"], "(kernel, device)", "hipFuncSetAttribute on the host, no stream involved", "n/a (a set of keys)",
         "the first launch of a kernel must not be inside a capture (the attribute call is not a stream operation); the launch tests run the kernel eagerly first",
         ["voxel_sorted"]),
    _rec("csrc/pointwise.hip ramnet_stream_fork", ["ramnet_stream_fork.ev"], "(host thread, device of `from`)",
         "hipEventCreateWithFlags on first use; recorded on `from` and waited for on `to` in the same call", "re-recorded by every call (a wait refers to the record before it)",
         "record + wait are captured as a dependency", []),
    # ---- package state (rpg_ramnet_amd/)
    _rec("metrics._workspaces", ["metrics._workspaces"], "(device index, raw stream)", "torch.empty + zero_() of the ticket bytes on the current stream, at allocation",
         "every kernel that draws a ticket puts it back", "not taken under a capture (no documented capture path)", ["batch_metrics"]),
    _rec("metrics._eval_workspaces", ["metrics._eval_workspaces"], "(device index, raw stream)", "torch.empty + zero_() of the ticket bytes on the current stream, at allocation",
         "every kernel that draws a ticket puts it back", "not taken under a capture (no documented capture path)", ["eval_table"]),
    _rec("metrics._tables", ["metrics._tables"], "(device index, raw stream, pointers of the pairs)",
         "pinned host tensor uploaded with non_blocking=True on the current stream: complete only in that stream's order", "n/a (read only); cleared at 256 entries",
         "not taken under a capture (no documented capture path)", ["batch_metrics"]),
    _rec("render._workspaces", ["render._workspaces"], "(device index, raw stream)", "torch.empty + zero_() of the ticket bytes on the current stream, at allocation",
         "rd_stats_kernel's last workgroup puts the tickets back", "not taken under a capture (no documented capture path)", ["render"]),
    _rec("render.ColorMapper._tables", ["ColorMapper._tables"], "device (per mapper object)", "a pageable .to(device): complete when the call returns, so ordered before any later launch",
         "n/a (read only)", "the upload must have happened before the capture (a pageable copy synchronises)", ["render"]),
    _rec("ops._msg_tables", ["ops._msg_tables"], "(device index, raw stream, pointers of the pairs)",
         "ramnet_fill_pointer_table by kernel argument on the current stream: complete only in that stream's order", "n/a (read only); cleared at 256 entries",
         "a capture never takes a table from the cache nor leaves one: it records a fill of its own", ["grad_loss_batch"]),
    _rec("ops._msg_workspaces", ["ops._msg_workspaces"], "(device index, raw stream)", "torch.empty; never initialised: gl_stats_kernel writes every slot gl_join_kernel reads",
         "nothing to reset (no tickets)", "a capture gets a torch.empty of its own (owned by the graph's pool), the cache is left alone", ["grad_loss_batch"]),
    _rec("ops._msg_weight_cache", ["ops._msg_weight_cache"], "(device index, tuple of weights)", "torch.tensor(..., device=): a pageable upload, complete when the call returns",
         "n/a (read only, never evicted: a captured graph may read it)", "the upload must have happened before the capture", ["grad_loss_batch"]),
    _rec("ops._CONSTS", ["ops._CONSTS"], "(name, device, dtype)", "torch.tensor(..., device=): a pageable upload, complete when the call returns", "n/a (read only)",
         "the upload must have happened before the capture", []),
    _rec("ops._S2D_ADJ_IDX", ["ops._S2D_ADJ_IDX"], "device", "torch.tensor(..., device=): a pageable upload, complete when the call returns", "n/a (read only)",
         "the upload must have happened before the capture", []),
    _rec("augment._coords", ["augment._coords"], "(H, W, device)", "two pageable .to(device): complete when the call returns", "n/a (read only)",
         "the upload must have happened before the capture", ["augment"]),
    _rec("augment._ptrs", ["augment._ptrs"], "(device, base pointer, G, stride in bytes)", "a pageable .to(device): complete when the call returns",
         "n/a (read only); cleared at 256 entries", "the upload must have happened before the capture", ["augment"]),
    # ---- layer-owned state: the documented contract only (history_cases.row_user_stream runs it)
    _rec("ConvParam packs", ["ConvParam.packs"], "layer", LAYER_CONTRACT, "re-packed when the weight's version moves", LAYER_CONTRACT, []),
    _rec("ConvParam._splitk", ["ConvParam._splitk"], "layer", LAYER_CONTRACT, "the split-K kernels put their counters back", LAYER_CONTRACT, ["conv_splitk"]),
    _rec("ConvParam._part", ["ConvParam._part"], "layer", LAYER_CONTRACT, "overwritten by every pass", LAYER_CONTRACT, []),
    _rec("gradient workspaces", ["ConvParam gradient workspaces"], "layer", LAYER_CONTRACT, "zeroed by the record's own zero step", LAYER_CONTRACT, []),
]

# module-level dicts / lists of the package that hold no device memory a launch reads: "<module>.<name>" -> why
NOT_DEVICE_STATE = {
    "ops._SWITCHES": "the table of switches: host configuration",
    "ops._ON_OFF": "a constant mapping of the switch table",
    "ops._ACT_CODE": "a constant mapping of activation names to codes",
    "ops._LAYOUTS": "the constant table of weight-gradient layouts",
    "ops._FOLD_LAYOUTS": "the constant table of the folded decoders' layouts",
    "ops._PACKS": "the constant table of pack kinds (the packs themselves are layer-owned)",
    "ops._FOLD_WGRAD_VARIANT": "host-side choice of a kernel variant per shape",
    "ops._ADDRESSABLE": "host-side answers of the size guards per shape",
    "ops._DESC_CACHE": "ctypes descriptors on the host; the stream is an argument of the launch, not of the descriptor",
    "ops._WDESC_CACHE": "ctypes descriptors on the host; the stream is an argument of the launch, not of the descriptor",
    "ops._DET_SLAB_QUERIES": "host-side answers of library queries",
    "ops._SIDE": "torch streams themselves (the backward-weights side stream), forked from and joined to the caller's stream by every pass",
    "ops._DECODE": "torch streams themselves (decoder overlap), joined by every pass",
    "ops._BRANCH": "torch streams themselves (branch overlap), joined by every pass",
}

# static containers / thread_local objects of csrc/ that are no device state: (file, identifier) -> why
CSRC_NOT_DEVICE_STATE = {
    ("pointwise.hip", "g_err"): "the last error message of the host thread",
    ("pointwise.hip", "g_kernel"): "the last kernel name of the host thread",
}
# (file, identifier) -> the record's name it belongs to
CSRC_RECORDED = {
    ("loss_voxel.hip", "bufs"): ("si_scratch.bufs", "voxel_id_scratch.bufs"),
    ("pointwise.hip", "done"): ("allow_full_lds.done",),
    ("pointwise.hip", "ev"): ("ramnet_stream_fork.ev",),
}

# ---- the rows: (surface, kind), run by tests/stream_worker.py in this order, each on a torch.cuda.Stream() of its own.
# library: the surface's state is library scratch (its own hipMalloc may order the device: `conclusive` is reported, not asserted)
SURFACES = {
    "si_loss": dict(library=True, entry="ramnet_si_loss_fwd", shape="n = 4099"),
    "si_log_loss": dict(library=True, entry="ramnet_si_log_loss_fwd", shape="n = 4099"),
    "mse_loss": dict(library=False, entry="ramnet_mse_loss_fwd", shape="2 x 33 x 31"),
    "voxel_sorted": dict(library=True, entry="ramnet_voxelize_batch_sorted", shape="voxel_cases m2: 1 x 40 x 9, lists of 0 and 300 events"),
    "batch_metrics": dict(library=False, entry="metrics.batch_metrics_table", shape="G = 3 pairs of metric_launch_cases (16, 8193): Ws = 2"),
    "eval_table": dict(library=False, entry="metrics.EvalTable.add (ramnet_eval_table_ex, masks, rescale)", shape="G = 3 maps of ET_CAP_ROWS first_at_cap: Ws = 32"),
    "render": dict(library=False, entry="render.render_package (ramnet_render_depth with scale pairs)", shape="64 x 257, G = 3, n_scale = 2"),
    "grad_loss_batch": dict(library=False, entry="ops.multi_scale_grad_loss_batch forward and backward", shape="grad_loss_cases m63x66_ns4: G = 3, two tiles per map"),
    "pred_sigmoid_si": dict(library=False, entry="ops.PredSigmoidSI (ramnet_pred_sigmoid_si_fwd / _bwd with scratch)", shape="C = 32, seg_pix = 517, nseg = 2"),
    "augment": dict(library=False, entry="augment.apply with stats= and scale_factor", shape="augment_scale_cases FAST: 40 x 56 -> 32 x 32 windows at 0.5, G = 4, 5 bins"),
    "conv_splitk": dict(library=False, entry="ramnet_conv_launch with splitk_ws", shape="test_wino_split_reduction: 9 x 11, Cin 32, wino_ksplit 2"),
}
# surfaces whose launches keep nothing beyond the call (no record points at them): why they have rows all the same
STATELESS = {
    "mse_loss": "zero-fills `stats` and adds to it atomically in every call: the issue's table lists it beside the SI losses",
    "pred_sigmoid_si": "its scratch is a torch.zeros of the call, handed from the forward to the backward launch: zeroed and used on the current stream",
}
KINDS = ("first_use", "second_use", "two_streams", "table_owner", "capture")
ROWS = [
    ("si_loss", "first_use"), ("si_loss", "second_use"), ("si_loss", "two_streams"), ("si_loss", "capture"),
    ("si_log_loss", "first_use"), ("si_log_loss", "second_use"), ("si_log_loss", "two_streams"),
    ("mse_loss", "first_use"), ("mse_loss", "second_use"), ("mse_loss", "two_streams"), ("mse_loss", "capture"),
    ("voxel_sorted", "first_use"), ("voxel_sorted", "second_use"), ("voxel_sorted", "two_streams"), ("voxel_sorted", "capture"),
    ("batch_metrics", "first_use"), ("batch_metrics", "second_use"), ("batch_metrics", "two_streams"), ("batch_metrics", "table_owner"),
    ("eval_table", "first_use"), ("eval_table", "second_use"), ("eval_table", "two_streams"), ("eval_table", "table_owner"),
    ("render", "first_use"), ("render", "second_use"), ("render", "two_streams"), ("render", "table_owner"),
    ("grad_loss_batch", "first_use"), ("grad_loss_batch", "second_use"), ("grad_loss_batch", "two_streams"), ("grad_loss_batch", "table_owner"),
    ("grad_loss_batch", "capture"),
    ("pred_sigmoid_si", "first_use"), ("pred_sigmoid_si", "second_use"), ("pred_sigmoid_si", "two_streams"),
    ("augment", "first_use"), ("augment", "second_use"), ("augment", "two_streams"),
    ("conv_splitk", "first_use"), ("conv_splitk", "second_use"),       # (self-resetting counters in a caller's workspace: these two kinds only)
]


def row_id(row):
    return "%s-%s" % row
