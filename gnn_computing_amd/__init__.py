"""gnn_computing_amd -- MI355X-native neighbor aggregation (GCN/GraphSAGE SpMM, GAT edge-softmax
SDDMM + SpMM) behind the reference's Aggregator API.  All compute is in libgnnagg.so (HIP, gfx950);
this package is the host-side mirror of the reference's operator interface plus input generators.
"""
from . import _lib
from ._lib import GnnAggError, lib  # noqa: F401
from .aggregator import (  # noqa: F401
    Aggregator, Aggregator_GAT, Aggregator_GCN, Schedule,
    gat_init, gat_run, gat_run_add_to_center, gat_run_div_each, gat_run_u_add_v, gat_schedule,
    gcn_init, gcn_run, gcn_schedule, gcn_update_val, new_load, load_graph_host,
    reorder_csr, neighbor_grouping_schedule, locality_schedule, partition_rows, halo_plan, cluster_reorder, matmul_NN,
    gat_project, last_project_path, gatv2_run, dot_attn_run, gcn_run_multi, pna_delta,
)
from .sampling import (  # noqa: F401
    Block, NeighborSampler, block_attn_run, block_gcn_run, block_sage_run, block_sage_supported, sage_prefers_fused, sample_block_host,
    block_sage_wide_supported, sage_prefers_wide,
    block_rgcn_run, block_rgcn_supported, rgcn_prefers_fused,
    block_rgcn_basis_run, block_rgcn_basis_supported, rgcn_basis_prefers_fused,
    block_gin_run, block_gin_supported, gin_prefers_fused,
    block_pna_run, block_pna_supported, pna_prefers_fused,
    block_edgeconv_run, block_edgeconv_supported, edgeconv_prefers_fused,
)
from .scoring import pair_score, pair_score_supported, pair_score_prefers_fused  # noqa: F401
from .knn import knn_graph, knn_run, knn_out_ptr, knn_supported, knn_prefers_fused, knn_work_bytes  # noqa: F401
from . import graph  # noqa: F401
from . import probe  # noqa: F401
# (gnn_computing_amd.extras -- torch.autograd wrappers over the backward entry points -- needs libgnnagg_extras.so: out of scope per
# SURVEY 2.2, not imported here)
