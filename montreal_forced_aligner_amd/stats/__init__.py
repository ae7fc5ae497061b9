"""The statistics stages of the host layer, each a device call and the host twin it is held to.  Functions of an engine, not
methods: they use its ``lib``, ``ctx``, ``device``, ``_dev``, the loaded ``gmm`` and its ``_launch_*`` calls.

  ``alignment``  what is computed from alignments: the shared tables (``model_arrays``, ``tid_tables``, ``silence_weights``,
                 ``check_delta_fmllr``), fMLLR statistics, ``GmmStats`` and the GMM statistics, LDA, MLLT and tree statistics
  ``speaker``    the diagonal UBM (Gaussian selection, global statistics) and the i-vector extractor (pruning, utterance
                 statistics, E-step)
  ``pairs``      the PLDA transform, the sweep for any metric and its consumers (scores, best, k-NN, neighbour bits),
                 ``dbscan_from_bits``, HDBSCAN's pair form, core scores and spanning tree, and the silhouette coefficients
  ``_common``    what their wrappers share: the device-model cache, ``GmmStats`` to accumulators and back, frame tables

A new stage goes into the module of its role (or a new one beside them) and is re-exported here; code inside the package
imports from the module that defines the name.
"""
from .alignment import (TREE_MAX_CLASSES, TREE_MAX_PHONES, TREE_NO_KEY, GmmStats, LdaStats, MlltStats, TreeStats,   # noqa: F401
                        check_delta_fmllr, fmllr_statistics, gaussian_means, gmm_statistics, gmm_statistics_host,
                        gmm_statistics_twofeats, gmm_statistics_twofeats_host, lda_statistics, lda_statistics_host, mllt_statistics,
                        mllt_statistics_host, model_arrays, silence_weights, tid_tables, tree_key, tree_statistics,
                        tree_statistics_host, tree_tid_tables)
from .pairs import (METRIC_CODES, NEIGHBOR_BITS_BYTES, PLDA_BLOCK_BYTES, PLDA_MATRIX_BYTES, _plda_score_call, _unit_rows,   # noqa: F401
                    core_scores, core_scores_host, dbscan_from_bits, dbscan_from_bits_host, finish_tree, knn, knn_host, metric_code,
                    metric_sweep, metric_sweep_host, mreach_mst, mreach_mst_host, neighbor_bits, neighbor_bits_host, pair_metric,
                    pair_prepare, pair_prepare_host, plda_classify, plda_classify_host, plda_knn, plda_knn_host, plda_prepare_host,
                    plda_scores, plda_scores_host, plda_sweep, plda_sweep_host, plda_transform, plda_transform_host, score_threshold,
                    score_to_distance, silhouette, silhouette_host)
from .speaker import (gaussian_selection, gaussian_selection_host, ivector_estep, ivector_estep_host,   # noqa: F401
                      ivector_utterance_statistics, ivector_utterance_statistics_host, prune_posteriors, prune_posteriors_host,
                      ubm_statistics, ubm_statistics_host)
