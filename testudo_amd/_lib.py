"""ctypes binding of libtpst.so (include/tpst.h).

The library is built in-tree by testudo_amd/build.py.  There is no CPU
fallback: if the shared object is missing or cannot be loaded, importing the
product path raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TPST_LIB_PATH") or os.path.join(_HERE, "libtpst.so")  # override: A/B builds (experiments)

_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p
_sz = C.c_size_t

# (name, restype, argtypes) -- mirrors include/tpst.h
PROTOTYPES = [
    ("tpst_device_count", C.c_int, []),
    ("tpst_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("tpst_destroy", None, [_vp]),
    ("tpst_last_error", C.c_char_p, [_vp]),
    ("tpst_stream", _vp, [_vp]),
    ("tpst_synchronize", C.c_int, [_vp]),
    ("tpst_wait_stream", C.c_int, [_vp, _vp]),
    ("tpst_join_stream", C.c_int, [_vp, _vp]),
    ("tpst_g1_msm", C.c_int, [_vp, _u64p, _sz, _u64p, _sz, _u64p]),
    ("tpst_g2_msm", C.c_int, [_vp, _u64p, _sz, _u64p, _sz, _u64p]),
    ("tpst_g1_msm_dev", C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("tpst_g1_msm_dev_async", C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("tpst_g1_msm_xyzz_dev", C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("tpst_g1_xyzz_sum_dev", C.c_int, [_vp, _vp, _sz, _sz, _vp]),
    ("tpst_g1_multiexp", C.c_int, [_vp, _u64p, _sz, _u64p, _sz, _u64p]),
    ("tpst_g2_multiexp", C.c_int, [_vp, _u64p, _sz, _u64p, _sz, _u64p]),
    ("tpst_gens_load", C.c_int, [_vp, _u64p, _sz, _u64p, C.POINTER(_vp)]),
    ("tpst_gens_free", None, [_vp]),
    ("tpst_gens_new", C.c_int, [_vp, _sz, C.c_char_p, _sz, _u64p, _u64p, C.POINTER(_vp)]),
    ("tpst_gens_seeds", C.c_int, [_sz, C.c_char_p, _sz, C.c_char_p]),
    ("tpst_g1_msm_batch", C.c_int, [_vp, _vp, _u64p, _sz, _sz, _sz, _sz, _u64p]),
    ("tpst_g1_msm_batch_dev", C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    ("tpst_pedersen_commit_slice", C.c_int, [_vp, _vp, _u64p, _sz, _u64p, _u64p]),
    ("tpst_pedersen_commit_rows", C.c_int, [_vp, _vp, _u64p, _sz, _u64p, _sz, _u64p]),
    ("tpst_g1_msm_fixed", C.c_int, [_vp, _u64p, _sz, _u64p, _sz, _sz, _u64p]),
    ("tpst_g2_msm_fixed", C.c_int, [_vp, _u64p, _sz, _u64p, _sz, _sz, _u64p]),
    ("tpst_multi_pairing", C.c_int, [_vp, _u64p, _u64p, _sz, _u64p]),
    ("tpst_g1_check", C.c_int, [_u64p]),
    ("tpst_g2_check", C.c_int, [_u64p]),
    ("tpst_g1_mul_generator", C.c_int, [_vp, _u64p, _sz, _u64p]),
    ("tpst_g2_mul_generator", C.c_int, [_vp, _u64p, _sz, _u64p]),
    ("tpst_g1_mul_generator_dev", C.c_int, [_vp, _vp, _sz, _vp]),
    ("tpst_microbench", C.c_int, [_vp, C.c_int, _sz, C.c_int, C.POINTER(C.c_double)]),
    ("tpst_microbench_wave_phases", C.c_int, [_vp, C.c_int, C.c_int, _u64p]),
    ("tpst_selftest_inv", C.c_int, [_vp, _sz, _u64p, _u64p, _u64p]),
    ("tpst_selftest_field", C.c_int, [_vp, C.c_int, _sz, _u64p, _u64p, _u64p]),
    ("tpst_selftest_curve", C.c_int, [_vp, C.c_int, _sz, _u64p, _u64p, _u64p]),
    ("tpst_selftest_tower", C.c_int, [_vp, C.c_int, _sz, _u64p, _u64p, _u64p]),
    ("tpst_selftest_fbt", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _u64p, _sz, _u64p, _sz, _sz, _sz, _sz, _sz,
                                    C.POINTER(C.c_uint32), _sz, _sz, _u64p]),
    ("tpst_transcript_init", None, [_vp]),
    ("tpst_transcript_append_g1", C.c_int, [_vp, _u64p]),
    ("tpst_transcript_append_gt", C.c_int, [_vp, _u64p]),
    ("tpst_transcript_challenge", C.c_int, [_vp, _u64p]),
    ("tpst_srs_flat_len", _sz, [C.c_int]),
    ("tpst_srs_setup", C.c_int, [_vp, C.c_int, C.c_uint64]),
    ("tpst_srs_load", C.c_int, [_vp, C.c_int, _u64p]),
    ("tpst_srs_export", C.c_int, [_vp, _u64p]),
    ("tpst_fr_stream", C.c_uint64, [C.c_uint64, _sz, C.c_uint64, _u64p]),
    ("tpst_poly_from_evaluations", C.c_int, [_vp, _u64p, C.c_int, C.POINTER(_vp)]),
    ("tpst_poly_from_evaluations_dev", C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    ("tpst_poly_from_evaluations_cols", C.c_int, [_vp, _u64p, C.c_int, _sz, _sz, C.POINTER(_vp)]),
    ("tpst_poly_free", None, [_vp]),
    ("tpst_poly_eval", C.c_int, [_vp, _vp, _u64p, _u64p]),
    ("tpst_poly_commit", C.c_int, [_vp, _vp, _u64p, _u64p]),
    ("tpst_poly_commit_dev", C.c_int, [_vp, _vp, _vp, _vp]),
    ("tpst_poly_commit_rows", C.c_int, [_vp, _vp, _sz, _sz, _u64p]),
    ("tpst_poly_ipp", C.c_int, [_vp, C.c_int, _u64p, _u64p]),
    ("tpst_poly_commit_rows_partial", C.c_int, [_vp, _vp, _sz, _sz, _u64p, _u64p]),
    ("tpst_gt_final_exp_product", C.c_int, [_vp, _u64p, _sz, _u64p]),
    ("tpst_poly_commit_rows_partial_dev", C.c_int, [_vp, _vp, _sz, _sz, _vp]),
    ("tpst_gt_final_exp_product_dev", C.c_int, [_vp, _vp, _sz, _sz, _u64p]),
    ("tpst_poly_get_q_partial", C.c_int, [_vp, _vp, _u64p, _sz, _sz, _u64p]),
    ("tpst_poly_get_q_partial_dev", C.c_int, [_vp, _vp, _u64p, _sz, _sz, _vp]),
    ("tpst_fr_sum_dev", C.c_int, [_vp, _vp, _sz, _sz, _vp]),
    ("tpst_poly_cu_partial", C.c_int, [_vp, C.c_int, _u64p, _sz, _sz, _u64p, _u64p]),
    ("tpst_poly_from_q_dev", C.c_int, [_vp, C.c_int, _u64p, _vp, _u64p, C.POINTER(_vp)]),
    ("tpst_poly_open", C.c_int, [_vp, _vp, _vp, _u64p, _u64p, _u64p, _vp]),
    ("tpst_open_sharded_arena_bytes", _sz, [C.c_int, C.c_int]),
    ("tpst_poly_open_sharded", C.c_int, [_vp, _vp, _vp, C.c_int, _u64p, _u64p, _u64p, _vp, _vp]),
    ("tpst_pst_verify", C.c_int, [_vp, _vp, C.c_int, _u64p, _u64p, _u64p, _vp]),
    ("tpst_pst_verify_batch", C.c_int, [_vp, C.c_int, _vp, _sz, _u64p, C.POINTER(C.c_uint8)]),
    ("tpst_poly_lincomb", C.c_int, [_vp, C.POINTER(_vp), _sz, _u64p, C.POINTER(_vp)]),
    ("tpst_poly_evaluations", C.c_int, [_vp, _vp, _u64p]),
    ("tpst_g1_lincomb_rows", C.c_int, [_vp, C.POINTER(_u64p), _sz, _sz, _u64p, _u64p]),
    ("tpst_commit_lincomb", C.c_int, [_vp, C.c_int, C.POINTER(_u64p), C.POINTER(_u64p), _sz, _u64p, _u64p, _u64p]),
    ("tpst_pst_combine_challenge", C.c_int, [_vp, C.c_int, _u64p, C.POINTER(_u64p), _u64p, _sz, _u64p]),
    ("tpst_poly_open_combined", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_u64p), C.POINTER(_u64p), _sz, _u64p, _vp,
                                          _u64p, _u64p, _u64p, _u64p, _vp]),
    ("tpst_pst_verify_combined", C.c_int, [_vp, _vp, C.c_int, _u64p, _u64p, C.POINTER(_u64p), _sz, _u64p, _vp]),
    ("tpst_poly_open_multi", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_u64p), C.POINTER(_u64p), _sz,
                                       C.POINTER(C.c_uint32), _u64p, _u64p, _sz, _vp, _u64p, _u64p, _u64p, _u64p, _u64p,
                                       _u64p, _vp]),
    ("tpst_pst_multi_reduce", C.c_int, [_vp, C.c_int, C.POINTER(_u64p), _sz, C.POINTER(C.c_uint32), _u64p, _u64p, _sz,
                                        _u64p, _u64p, _u64p]),
    ("tpst_pst_verify_multi", C.c_int, [_vp, _vp, C.c_int, C.POINTER(_u64p), _sz, C.POINTER(C.c_uint32), _u64p, _u64p,
                                        _sz, _u64p, _u64p, _vp]),
    ("tpst_poly_multi_sumcheck_stages", C.c_int, [_vp, C.POINTER(_vp), _sz, C.POINTER(C.c_uint32), _u64p, _u64p, _sz,
                                                  _u64p, _u64p, _u64p]),
    # terms: a (tpst_sc_term * M) array, handed over as void*
    ("tpst_poly_sumcheck_open", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_u64p), C.POINTER(_u64p), _sz, _vp, _sz, _u64p,
                                          _vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _vp]),
    ("tpst_pst_sumcheck_reduce", C.c_int, [_vp, C.c_int, C.POINTER(_u64p), _sz, _vp, _sz, _u64p, _u64p, _u64p, _u64p,
                                           _u64p]),
    ("tpst_pst_verify_sumcheck", C.c_int, [_vp, _vp, C.c_int, C.POINTER(_u64p), _sz, _vp, _sz, _u64p, _u64p, _u64p,
                                           _u64p, _vp]),
    ("tpst_poly_sumcheck_stages", C.c_int, [_vp, C.POINTER(_vp), _sz, _vp, _sz, _u64p, _u64p, _u64p, _u64p]),
    ("tpst_poly_lookup_open", C.c_int, [_vp, C.POINTER(_vp), _sz, _vp, C.POINTER(_u64p), C.POINTER(_u64p), _vp, _u64p,
                                        _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _vp]),
    ("tpst_pst_lookup_reduce", C.c_int, [_vp, C.c_int, _sz, C.POINTER(_u64p), _u64p, _u64p, _u64p, _u64p, _u64p, _u64p,
                                         _u64p]),
    ("tpst_pst_verify_lookup", C.c_int, [_vp, _vp, C.c_int, _sz, C.POINTER(_u64p), _u64p, _u64p, _u64p, _u64p, _u64p,
                                         _u64p, _vp]),
    ("tpst_poly_lookup_stages", C.c_int, [_vp, C.POINTER(_vp), _sz, _vp, _u64p, _u64p, _u64p, _u64p]),
    ("tpst_mlpc_commit", C.c_int, [_vp, _u64p, C.c_int, _u64p]),
    ("tpst_mlpc_commit_g2", C.c_int, [_vp, _u64p, C.c_int, _u64p]),
    ("tpst_mlpc_open", C.c_int, [_vp, _u64p, C.c_int, _u64p, _u64p]),
    ("tpst_mlpc_open_g1", C.c_int, [_vp, _u64p, C.c_int, _u64p, _u64p]),
    ("tpst_mlpc_check", C.c_int, [_vp, C.c_int, _u64p, _u64p, _u64p, _u64p]),
    ("tpst_mlpc_check_2", C.c_int, [_vp, C.c_int, _u64p, _u64p, _u64p, _u64p]),
    ("tpst_transcript_append_fr", C.c_int, [_vp, _u64p]),
    ("tpst_transcript_reset_fr", C.c_int, [_vp, _u64p]),
    ("tpst_transcript_append_bytes", C.c_int, [_vp, C.c_char_p, _sz]),
    ("tpst_unipoly_from_evals", C.c_int, [_u64p, C.c_int, _u64p]),
    ("tpst_eq_evals", C.c_int, [_vp, _u64p, C.c_int, _u64p]),
    ("tpst_r1cs_load", C.c_int, [_vp, _sz, _sz, _sz, C.POINTER(_sz), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                 C.POINTER(_vp)]),
    ("tpst_r1cs_synthetic", C.c_int, [_vp, _sz, _sz, _sz, C.c_uint64, C.POINTER(_vp), _u64p, _u64p]),
    ("tpst_r1cs_free", None, [_vp]),
    ("tpst_r1cs_commit", C.c_int, [_vp, _vp, C.c_char_p, _sz, _u64p, C.POINTER(_sz), _u64p, C.POINTER(_sz)]),
    ("tpst_r1cs_prove", C.c_int, [_vp, _vp, _u64p, _u64p, _vp, _vp]),
    ("tpst_r1cs_evaluate", C.c_int, [_vp, _vp, _u64p, _u64p, _u64p]),
    ("tpst_r1cs_is_sat", C.c_int, [_vp, _vp, _u64p, _u64p]),
    ("tpst_r1cs_verify_evals", C.c_int, [_vp, _sz, _sz, _u64p, _sz, _u64p, _vp, _vp]),
    ("tpst_r1cs_verify", C.c_int, [_vp, _vp, _u64p, _vp, _vp]),
    ("tpst_transcript_fr_init", None, [_vp]),
    ("tpst_transcript_fr_append_scalar", C.c_int, [_vp, _u64p]),
    ("tpst_transcript_fr_append_scalars", C.c_int, [_vp, _u64p, _sz]),
    ("tpst_transcript_fr_append_point", C.c_int, [_vp, _u64p]),
    ("tpst_transcript_fr_append_bytes", C.c_int, [_vp, C.c_char_p, _sz]),
    ("tpst_transcript_fr_challenge", C.c_int, [_vp, _u64p]),
    ("tpst_dotprod_prove", C.c_int, [_vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _vp, _vp, _u64p,
                                     _u64p]),
    ("tpst_dotprod_verify", C.c_int, [_vp, _vp, _u64p, _u64p, _u64p, _u64p, _vp, _vp]),
    ("tpst_hyrax_eval_prove", C.c_int, [_vp, _vp, _u64p, _u64p, C.c_int, _u64p, _u64p, _u64p, _u64p, _u64p, _vp, _vp,
                                        _u64p]),
    ("tpst_hyrax_eval_prove_dev", C.c_int, [_vp, _vp, _u64p, _vp, C.c_int, _u64p, _u64p, _u64p, _u64p, _u64p, _vp,
                                            _vp, _u64p]),
    ("tpst_hyrax_eval_verify", C.c_int, [_vp, _vp, _u64p, C.c_int, _u64p, _u64p, _u64p, _vp, _vp]),
    ("tpst_hyrax_eval_verify_plain", C.c_int, [_vp, _vp, _u64p, C.c_int, _u64p, _u64p, _u64p, _vp, _vp]),
    ("tpst_dense_evaluate", C.c_int, [_vp, _u64p, C.c_int, _u64p, _u64p]),
    ("tpst_prodcircuit_proof_len", _sz, [C.c_int, _sz, _sz]),
    ("tpst_prodcircuit_prove", C.c_int, [_vp, C.c_int, _sz, _u64p, _sz, _u64p, _u64p, _u64p, _vp, _u64p, _u64p,
                                         _u64p, _u64p]),
    ("tpst_prodcircuit_prove_dev", C.c_int, [_vp, C.c_int, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _u64p, _u64p, _u64p,
                                             _u64p]),
    ("tpst_prodcircuit_verify", C.c_int, [C.c_int, _sz, _sz, _u64p, _u64p, _u64p, _vp, _u64p, _u64p, _u64p]),
    ("tpst_r1cs_gens_setup", C.c_int, [_vp, C.c_char_p, _sz, _sz, _sz, _sz, _sz, C.POINTER(_vp)]),
    ("tpst_r1cs_gens_free", None, [_vp]),
    ("tpst_r1cs_commit_decomm", C.c_int, [_vp, _vp, _vp, _u64p, C.POINTER(_sz), _u64p, C.POINTER(_sz),
                                          C.POINTER(_vp)]),
    ("tpst_r1cs_decomm_free", None, [_vp]),
    ("tpst_r1cs_eval_proof_sizes", C.c_int, [_sz, _sz, _sz, _vp]),
    ("tpst_r1cs_eval_prove", C.c_int, [_vp, _vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _vp, _vp, _u64p,
                                       _u64p, _u64p]),
    ("tpst_r1cs_eval_verify", C.c_int, [_vp, _u64p, _u64p, _sz, _sz, _vp, _u64p, _u64p, _u64p, _vp, _vp, _u64p,
                                        _u64p, _u64p]),
    ("tpst_r1cs_eval_stages", C.c_int, [_vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("tpst_transcript_fr_append_u64", C.c_int, [_vp, C.c_uint64]),
    ("tpst_transcript_fr_new_from_state", C.c_int, [_vp, _u64p]),
    ("tpst_r1cs_commitment_absorb", C.c_int, [_vp, _vp]),
    ("tpst_snark_prove", C.c_int, [_vp, _vp, _vp, _vp, _vp, _u64p, _sz, _u64p, _u64p, _u64p, _u64p, _vp, _vp, _u64p,
                                   _u64p, _u64p]),
    ("tpst_snark_verify", C.c_int, [_vp, _vp, _vp, _u64p, _sz, _vp, _vp, _u64p, _u64p, _u64p]),
    ("tpst_nizk_prove", C.c_int, [_vp, _vp, C.c_char_p, _sz, _u64p, _sz, _u64p, _vp, _vp]),
    ("tpst_nizk_verify", C.c_int, [_vp, _vp, C.c_char_p, _sz, _u64p, _vp, _vp]),
    ("tpst_groth16_setup", C.c_int, [_vp, _vp, _u64p, C.POINTER(_vp)]),
    ("tpst_groth16_pk_free", None, [_vp]),
    ("tpst_groth16_domain", C.c_int, [_vp, C.POINTER(_sz)]),
    ("tpst_groth16_vk", C.c_int, [_vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("tpst_groth16_witness_map", C.c_int, [_vp, _vp, _vp, _u64p, _u64p, _u64p]),
    ("tpst_groth16_prove", C.c_int, [_vp, _vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("tpst_groth16_verify", C.c_int, [_vp, _u64p, _u64p, _u64p, _u64p, _u64p, _sz, _u64p, _sz, _u64p, _u64p,
                                      _u64p]),
    ("tpst_ser_g1", C.c_int, [_u64p, C.c_char_p]),
    ("tpst_ser_g2", C.c_int, [_u64p, C.c_char_p]),
    ("tpst_de_g1", C.c_int, [C.c_char_p, _u64p]),
    ("tpst_de_g2", C.c_int, [C.c_char_p, _u64p]),
    ("tpst_ser_commitment", C.c_int, [C.c_int, _u64p, C.c_char_p, _sz, C.POINTER(_sz)]),
    ("tpst_ser_pst_proof", C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(_sz)]),
    ("tpst_ser_mipp_proof", C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(_sz)]),
    ("tpst_de_open_proof", C.c_int, [C.c_char_p, _sz, C.c_char_p, _sz, _vp]),
    ("tpst_ser_committer_key", C.c_int, [C.c_int, _u64p, _sz, C.c_char_p, _sz, C.POINTER(_sz)]),
    ("tpst_de_g1_batch", C.c_int, [_vp, C.c_char_p, _sz, _u64p, C.POINTER(_sz)]),
    ("tpst_de_g2_batch", C.c_int, [_vp, C.c_char_p, _sz, _u64p, C.POINTER(_sz)]),
    ("tpst_g1_check_batch", C.c_int, [_vp, _u64p, _sz, C.POINTER(_sz)]),
    ("tpst_g2_check_batch", C.c_int, [_vp, _u64p, _sz, C.POINTER(_sz)]),
    ("tpst_g1_lincomb_batch", C.c_int, [_vp, _u64p, _u64p, _u64p, _u64p, _sz, _u64p]),
    ("tpst_g2_lincomb_batch", C.c_int, [_vp, _u64p, _u64p, _u64p, _u64p, _sz, _u64p]),
    ("tpst_ser_r1cs_commitment", C.c_int, [_sz, _sz, _sz, _sz, _sz, _u64p, _sz, _u64p, _sz, C.c_char_p, _sz,
                                           C.POINTER(_sz)]),
    ("tpst_de_r1cs_commitment", C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(_sz), _u64p, _sz, C.POINTER(_sz), _u64p,
                                          _sz, C.POINTER(_sz)]),
    ("tpst_ser_r1cs_eval_proof", C.c_int, [_vp, _vp, _u64p, _u64p, _u64p, C.c_char_p, _sz, C.POINTER(_sz)]),
    ("tpst_de_r1cs_eval_proof", C.c_int, [_vp, C.c_char_p, _sz, _vp, _vp, _u64p, _u64p, _u64p]),
    ("tpst_ser_r1cs_proof", C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(_sz)]),
    ("tpst_de_r1cs_proof", C.c_int, [_vp, C.c_char_p, _sz, _sz, _sz, _vp]),
    ("tpst_ser_snark_proof", C.c_int, [_vp, _vp, _u64p, _u64p, _u64p, C.c_char_p, _sz, C.POINTER(_sz)]),
    ("tpst_de_snark_proof", C.c_int, [_vp, C.c_char_p, _sz, _sz, _sz, _vp, _vp, _u64p, _u64p, _u64p]),
    ("tpst_de_committer_key", C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(C.c_int), _u64p, _sz, C.POINTER(_sz)]),
    ("tpst_profile_enable", C.c_int, [_vp, C.c_int]),
    ("tpst_profile_reset", C.c_int, [_vp]),
    ("tpst_profile_read", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
]

MAX_VARS = 20


class Transcript(C.Structure):
    """tpst_transcript: PoseidonTranscript<Fq> sponge state."""
    _fields_ = [("state", (C.c_uint64 * 6) * 3), ("squeezing", C.c_uint32), ("index", C.c_uint32)]


class OpenProof(C.Structure):
    """tpst_open_proof: (U, PST proof, MippProof) of Polynomial::open."""
    _fields_ = [
        ("m_col", C.c_int32), ("m_row", C.c_int32),
        ("U", C.c_uint64 * 12),
        ("pst_proof", (C.c_uint64 * 24) * MAX_VARS),
        ("comms_t", ((C.c_uint64 * 72) * 2) * MAX_VARS),
        ("comms_u", ((C.c_uint64 * 12) * 2) * MAX_VARS),
        ("final_a", C.c_uint64 * 12),
        ("final_h", C.c_uint64 * 24),
        ("pst_proof_h", (C.c_uint64 * 12) * MAX_VARS),
    ]

class ScTerm(C.Structure):
    """tpst_sc_term: one term c prod_i f_idx[i] of a product sum-check."""
    _fields_ = [("deg", C.c_uint32), ("idx", C.c_uint32 * 3), ("coeff", C.c_uint64 * 4)]


class VerifyItem(C.Structure):
    """tpst_verify_item: one opening of tpst_pst_verify_batch."""
    _fields_ = [("point", _u64p), ("v", _u64p), ("T", _u64p), ("proof", C.POINTER(OpenProof)),
                ("tr", C.POINTER(Transcript))]


# tpst_allgather_fn(user, send_off, recv_off, bytes, stream) -> 0 on success
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, _vp, _sz, _sz, _sz, _vp)


class Exchange(C.Structure):
    """tpst_exchange: the caller's all-gather for tpst_poly_open_sharded."""
    _fields_ = [("world", C.c_int), ("rank", C.c_int), ("allgather", ALLGATHER_FN), ("user", _vp),
                ("d_arena", _vp), ("arena_bytes", _sz)]


R1CS_MAX_ROUNDS = 48


class R1CSProof(C.Structure):
    """tpst_r1cs_proof: R1CSProof (r1csproof.rs:24-38) without the Groth16 part."""
    _fields_ = [
        ("rounds_x", C.c_int32), ("rounds_y", C.c_int32), ("num_vars_log", C.c_int32), ("pad", C.c_int32),
        ("T", C.c_uint64 * 72),
        ("initial_state", C.c_uint64 * 4),
        ("sc1", ((C.c_uint64 * 4) * 4) * R1CS_MAX_ROUNDS),
        ("claims_phase2", (C.c_uint64 * 4) * 4),
        ("claims_phase2_z_abc", (C.c_uint64 * 4) * 2),
        ("r_abc", (C.c_uint64 * 4) * 3),
        ("sc2", ((C.c_uint64 * 4) * 3) * R1CS_MAX_ROUNDS),
        ("rx", (C.c_uint64 * 4) * R1CS_MAX_ROUNDS),
        ("ry", (C.c_uint64 * 4) * R1CS_MAX_ROUNDS),
        ("transcript_sat_state", C.c_uint64 * 4),
        ("eval_vars_at_ry", C.c_uint64 * 4),
        ("open", OpenProof),
    ]


HYRAX_MAX_ROUNDS = 16


class TranscriptFr(C.Structure):
    """tpst_transcript_fr: PoseidonTranscript<Fr> sponge state."""
    _fields_ = [("state", (C.c_uint64 * 4) * 3), ("squeezing", C.c_uint32), ("index", C.c_uint32)]


class DotProdProof(C.Structure):
    """tpst_dotprod_proof: DotProductProofLog (nizk/mod.rs:32-38)."""
    _fields_ = [
        ("rounds", C.c_int32), ("pad", C.c_int32),
        ("L", (C.c_uint64 * 12) * HYRAX_MAX_ROUNDS),
        ("R", (C.c_uint64 * 12) * HYRAX_MAX_ROUNDS),
        ("delta", C.c_uint64 * 12), ("beta", C.c_uint64 * 12),
        ("z1", C.c_uint64 * 4), ("z2", C.c_uint64 * 4),
    ]


class R1CSEvalProof(C.Structure):
    """tpst_r1cs_eval_proof: the fixed-size part of R1CSEvalProof."""
    _fields_ = [
        ("prod_row", (C.c_uint64 * 4) * 8), ("prod_col", (C.c_uint64 * 4) * 8),
        ("prod_val", ((C.c_uint64 * 4) * 3) * 2),
        ("hash_row", (C.c_uint64 * 4) * 7), ("hash_col", (C.c_uint64 * 4) * 7),
        ("hash_val", (C.c_uint64 * 4) * 3), ("hash_derefs", ((C.c_uint64 * 4) * 3) * 2),
        ("proof_derefs", DotProdProof), ("proof_ops", DotProdProof), ("proof_mem", DotProdProof),
    ]


class R1CSEvalSizes(C.Structure):
    """tpst_r1cs_eval_sizes"""
    _fields_ = [
        ("num_ops", _sz), ("num_mem_cells", _sz),
        ("ell_ops", C.c_int32), ("ell_mem", C.c_int32), ("ell_derefs", C.c_int32),
        ("log_ops", C.c_int32), ("log_cells", C.c_int32),
        ("ops_rows", _sz), ("mem_rows", _sz), ("derefs_rows", _sz),
        ("prod_ops_len", _sz), ("prod_mem_len", _sz),
        ("rnd_len", _sz * 3),
    ]


class R1CSCommitmentC(C.Structure):
    """tpst_r1cs_commitment: the dimensions and row lists of an R1CSCommitment."""
    _fields_ = [
        ("num_cons", _sz), ("num_vars", _sz), ("num_inputs", _sz), ("num_ops", _sz), ("num_mem_cells", _sz),
        ("comm_ops", _u64p), ("ops_rows", _sz), ("comm_mem", _u64p), ("mem_rows", _sz),
    ]


class SnarkProof(C.Structure):
    """tpst_snark_proof: (R1CSProof, inst_evals, the fixed part of R1CSEvalProof)."""
    _fields_ = [("sat", R1CSProof), ("inst_evals", (C.c_uint64 * 4) * 3), ("eval", R1CSEvalProof)]


_lib = None


def load() -> C.CDLL:
    """Load libtpst.so and bind every prototype; raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libtpst.so not built (%s); run testudo_amd/build.py" % LIB_PATH)
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 /
    # libhsa-runtime64.so.1.  Loaded first, it satisfies libtpst's
    # dependencies by soname; loaded after libtpst (which links /opt/rocm's),
    # both runtimes would initialise the device and torch finds no GPU --
    # and device pointers / streams could not be shared across the two.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, res, args in PROTOTYPES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return [p[0] for p in PROTOTYPES]
