"""
ctypes binding of librubiks_hip.so (C ABI: include/rubiks_hip.h).

The library is the product; this file only declares its entry points.  If the shared object is missing
the import of any compute module fails loudly -- there is deliberately no Python/NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (imported first so that librubiks_hip.so binds to the HIP runtime torch already loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librubiks_hip.so")

REPR_2024, REPR_686 = 0, 1
OH_F32, OH_F16, OH_BF16, OH_STATES, OH_I8 = 0, 1, 2, 3, 4
OHL_GATHER, OHL_MFMA, OHL_MFMA_DIRECT, OHL_MFMA_TILED = 0, 1, 2, 3
OHL_ACT_NONE, OHL_ACT_ELU, OHL_ACT_RELU = 0, 1, 2
INT64_MAX = (1 << 63) - 1

_vp, _sz, _i = C.c_void_p, C.c_size_t, C.c_int

#: name -> (restype, argtypes); kept in the order of include/rubiks_hip.h.  tests/test_abi.py checks that the
#: header, this table and the built library agree symbol for symbol.
SIGNATURES = {
	"rk_version": (_i, []),
	"rk_last_error": (C.c_char_p, []),
	"rk_init": (_i, [_i]),
	"rk_set_pacing": (_i, [_i]),
	"rk_calibrate_pacing": (_i, [_i]),
	"rk_get_pacing": (_i, [C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
	"rk_pace_slot_of_device": (_i, [_i]),
	"rk_stream_register": (_i, [_vp]),
	"rk_stream_forget": (_i, [_vp]),
	"rk_tables": (_i, [_i, _vp]),
	"rk_face_definitions": (_i, [_vp]),
	"rk_solved": (_i, [_i, _vp]),
	"rk_malloc": (_i, [C.POINTER(_vp), _sz]),
	"rk_free": (_i, [_vp]),
	"rk_memcpy_h2d": (_i, [_vp, _vp, _sz, _vp]),
	"rk_memcpy_d2h": (_i, [_vp, _vp, _sz, _vp]),
	"rk_memset": (_i, [_vp, _i, _sz, _vp]),
	"rk_stream_synchronize": (_i, [_vp]),
	"rk_multi_rotate": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
	"rk_multi_rotate_solved": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_bad_actions_seen": (_i, [C.POINTER(C.c_int), _vp]),
	"rk_multi_rotate_fd": (_i, [_i, _vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_expand12": (_i, [_i, _vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_expand12_soa": (_i, [_vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_states_to_soa": (_i, [_vp, _vp, _sz, _vp]),
	"rk_states_from_soa": (_i, [_vp, _vp, _sz, _vp]),
	"rk_multi_is_solved": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
	"rk_apply_sequences": (_i, [_i, _vp, _i, _i, _i, _i, _vp, _vp]),
	"rk_rollout_fanout": (_i, [_i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
	"rk_as_oh": (_i, [_i, _vp, _vp, _i, _sz, _vp]),
	"rk_ohl_create": (_i, [C.POINTER(_vp), _vp, _i, _vp, _i, _vp]),
	"rk_ohl_destroy": (_i, [_vp]),
	"rk_ohl_forward": (_i, [_vp, _vp, _vp, _i, _sz, _i, _vp]),
	"rk_ohl_set_epilogue": (_i, [_vp, _i, C.c_float, _vp, _vp, _vp]),
	"rk_ohl_set_weights": (_i, [_vp, _vp, _i, _vp, _vp]),
	"rk_ohl_backward": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
	"rk_ohl_backward_rows": (_sz, [_sz, _i]),
	"rk_tail_linear": (_i, [_vp, _sz, _i, _sz, _vp, _vp, _i, _i, C.c_float, _vp, _vp]),
	"rk_as_correct686": (_i, [_vp, _vp, _sz, _vp]),
	"rk_oh686_from2024": (_i, [_vp, _vp, _i, _sz, _vp]),
	"rk_686_to2024": (_i, [_vp, _vp, _vp, _sz, _vp]),
	"rk_astar_create": (_i, [C.POINTER(_vp), _sz, _i]),
	"rk_astar_destroy": (_i, [_vp]),
	"rk_astar_reset": (_i, [_vp, _vp, C.c_double, _vp]),
	"rk_astar_set_budget": (_i, [_vp, C.c_longlong, _vp]),
	"rk_astar_grow": (_i, [_vp, _sz, _vp]),
	"rk_astar_step_expand": (_i, [_vp, _vp, _i, _vp]),
	"rk_astar_step_commit": (_i, [_vp, _vp, _vp]),
	"rk_astar_set_values_dtype": (_i, [_vp, _i]),
	"rk_astar_status": (_i, [_vp, _vp, _vp]),
	"rk_astar_expand": (_i, [_vp, _i, _vp, _vp]),
	"rk_astar_new_states_oh": (_i, [_vp, _vp, _i, _vp]),
	"rk_astar_commit": (_i, [_vp, _vp, _vp]),
	"rk_astar_size": (C.c_longlong, [_vp]),
	"rk_astar_open_size": (C.c_longlong, [_vp]),
	"rk_astar_export": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
	"rk_astar_path": (C.c_longlong, [_vp, C.c_longlong, _vp, _sz, _vp]),
	"rk_astar_lookup": (C.c_longlong, [_vp, _vp, _vp]),
	"rk_astar_export_open": (C.c_longlong, [_vp, _vp, _vp, _sz, _vp]),
	"rk_astar_next_pops": (C.c_longlong, [_vp, _vp, _sz, _vp]),
	"rk_bfs_create": (_i, [C.POINTER(_vp), _sz, _i]),
	"rk_bfs_destroy": (_i, [_vp]),
	"rk_bfs_reset": (_i, [_vp, _vp, C.c_longlong, _vp]),
	"rk_bfs_set_budget": (_i, [_vp, C.c_longlong, _vp]),
	"rk_bfs_run": (_i, [_vp, _i, _vp]),
	"rk_bfs_status": (_i, [_vp, _vp, _vp]),
	"rk_bfs_grow": (_i, [_vp, _sz, _vp]),
	"rk_bfs_size": (C.c_longlong, [_vp]),
	"rk_bfs_export": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _vp]),
	"rk_bfs_path": (C.c_longlong, [_vp, _vp, _sz, _vp]),
	"rk_bibfs_create": (_i, [C.POINTER(_vp), _sz, _i]),
	"rk_bibfs_destroy": (_i, [_vp]),
	"rk_bibfs_reset": (_i, [_vp, _vp, C.c_longlong, _vp]),
	"rk_bibfs_run": (_i, [_vp, _i, _vp]),
	"rk_bibfs_status": (_i, [_vp, _vp, _vp]),
	"rk_bibfs_grow": (_i, [_vp, _sz, _vp]),
	"rk_bibfs_size": (C.c_longlong, [_vp]),
	"rk_bibfs_export": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
	"rk_bibfs_path": (C.c_longlong, [_vp, _vp, _sz, _vp]),
	"rk_ball_create": (_i, [C.POINTER(_vp), _i, _i]),
	"rk_ball_destroy": (_i, [_vp]),
	"rk_ball_build": (_i, [_vp, _i, _vp]),
	"rk_ball_status": (_i, [_vp, _vp]),
	"rk_ball_export": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _vp]),
	"rk_ball_depth": (_i, [_vp, _vp, _sz, _vp, _vp]),
	"rk_ball_solve": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
	"rk_bshorten_scratch_bytes": (C.c_longlong, [_sz, _i, _i]),
	"rk_bshorten": (_i, [_vp, _vp, _vp, _sz, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_bsearch_create": (_i, [C.POINTER(_vp), _vp, _sz, _i]),
	"rk_bsearch_destroy": (_i, [_vp]),
	"rk_bsearch_reset": (_i, [_vp, _vp, C.c_longlong, _vp]),
	"rk_bsearch_run": (_i, [_vp, _i, _vp]),
	"rk_bsearch_status": (_i, [_vp, _vp, _vp]),
	"rk_bsearch_grow": (_i, [_vp, _sz, _vp]),
	"rk_bsearch_size": (C.c_longlong, [_vp]),
	"rk_bsearch_export": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _vp]),
	"rk_bsearch_path": (C.c_longlong, [_vp, _vp, _sz, _vp]),
	"rk_bsearchb_create": (_i, [C.POINTER(_vp), _vp, _i, _sz, _i]),
	"rk_bsearchb_destroy": (_i, [_vp]),
	"rk_bsearchb_reset": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
	"rk_bsearchb_run": (_i, [_vp, _i, _vp]),
	"rk_bsearchb_status": (_i, [_vp, _vp, _vp]),
	"rk_bsearchb_paths": (_i, [_vp, _vp, _i, _vp]),
	"rk_bsearchb_export": (_i, [_vp, _i, _sz, _sz, _vp, _vp, _vp, _vp]),
	"rk_sym_tables": (_i, [_vp, _vp, _vp]),
	"rk_sym_canonical": (_i, [_vp, _sz, _vp, _vp, _vp, _vp]),
	"rk_sym_conjugate": (_i, [_vp, _sz, _i, _vp, _vp]),
	"rk_group_tables": (_i, [_vp, _vp, _vp]),
	"rk_group_apply": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
	"rk_group_inverse": (_i, [_vp, _sz, _vp, _vp]),
	"rk_group_relative": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
	"rk_group_legal": (_i, [_vp, _sz, _vp, _vp, _vp]),
	"rk_pdb_create": (_i, [C.POINTER(_vp), _vp, _i, _vp, _i]),
	"rk_pdb_destroy": (_i, [_vp]),
	"rk_pdb_build": (_i, [_vp, _vp]),
	"rk_pdb_status": (_i, [_vp, _vp]),
	"rk_pdb_export": (_i, [_vp, _sz, _sz, _vp, _vp]),
	"rk_pdb_depth": (_i, [_vp, _vp, _sz, _vp, _vp]),
	"rk_pdb_solve": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
	"rk_bound_create": (_i, [C.POINTER(_vp), _vp, _i]),
	"rk_bound_destroy": (_i, [_vp]),
	"rk_bound_depth": (_i, [_vp, _vp, _sz, _vp, _vp]),
	"rk_chain_create": (_i, [C.POINTER(_vp), _vp]),
	"rk_chain_destroy": (_i, [_vp]),
	"rk_chain_status": (_i, [_vp, _vp]),
	"rk_chain_export": (_i, [_vp, _i, _sz, _sz, _vp, _vp]),
	"rk_chain_solve": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
	"rk_twophase_create": (_i, [C.POINTER(_vp), _vp]),
	"rk_twophase_destroy": (_i, [_vp]),
	"rk_twophase_status": (_i, [_vp, _vp]),
	"rk_twophase_export": (_i, [_vp, _i, _sz, _sz, _vp, _vp]),
	"rk_twophase_solve": (_i, [_vp, _vp, _vp, _sz, _i, C.c_longlong, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
	"rk_twophase_solve_capped": (_i, [_vp, _vp, _vp, _sz, _i, C.c_longlong, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
	"rk_symball_create": (_i, [C.POINTER(_vp), _i, _i, _sz]),
	"rk_symball_destroy": (_i, [_vp]),
	"rk_symball_build": (_i, [_vp, _i, _vp]),
	"rk_symball_status": (_i, [_vp, _vp]),
	"rk_symball_export": (_i, [_vp, _sz, _sz, _vp, _vp]),
	"rk_symball_depth": (_i, [_vp, _vp, _sz, _vp, _vp]),
	"rk_symball_solve": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
	"rk_symball_child_values": (_i, [_vp, _vp, _sz, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_symball_child_values_scratch_bytes": (C.c_longlong, [_sz]),
	"rk_symball_state_at": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
	"rk_symball_index_status": (_i, [_vp, _vp]),
	"rk_symball_child_depths": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
	"rk_sdeepen": (_i, [_vp, _vp, _vp, _sz, _i, C.c_uint32, C.c_uint32, _vp, _vp]),
	"rk_sdeepen_max_probes": (C.c_longlong, []),
	"rk_sdeepen_pruned": (_i, [_vp, _vp, _vp, _vp, _sz, _i, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
	"rk_sshorten": (_i, [_vp, _vp, _vp, _sz, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_ssearch_create": (_i, [C.POINTER(_vp), _vp, _sz, _i]),
	"rk_ssearch_destroy": (_i, [_vp]),
	"rk_ssearch_reset": (_i, [_vp, _vp, C.c_longlong, _vp]),
	"rk_ssearch_run": (_i, [_vp, _i, _vp]),
	"rk_ssearch_status": (_i, [_vp, _vp, _vp]),
	"rk_ssearch_grow": (_i, [_vp, _sz, _vp]),
	"rk_ssearch_size": (C.c_longlong, [_vp]),
	"rk_ssearch_export": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _vp]),
	"rk_ssearch_path": (C.c_longlong, [_vp, _vp, _sz, _vp]),
	"rk_sdeepen_set_pops": (_i, [_vp, _i, _vp]),
	"rk_sdeepen_frontier": (_i, [_vp, _vp, _vp]),
	"rk_sdeepen_nodes": (_i, [_vp, _i, _sz, _sz, C.c_uint32, C.c_uint32, _vp, _vp]),
	"rk_sdeepen_nodes_pruned": (_i, [_vp, _vp, _i, _sz, _sz, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
	"rk_sdeepen_path": (C.c_longlong, [_vp, C.c_longlong, _i, C.c_uint32, _vp, _sz, _vp]),
	"rk_ssearchb_create": (_i, [C.POINTER(_vp), _vp, _i, _sz, _i]),
	"rk_ssearchb_destroy": (_i, [_vp]),
	"rk_ssearchb_reset": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
	"rk_ssearchb_run": (_i, [_vp, _i, _vp]),
	"rk_ssearchb_status": (_i, [_vp, _vp, _vp]),
	"rk_ssearchb_paths": (_i, [_vp, _vp, _i, _vp]),
	"rk_ssearchb_export": (_i, [_vp, _i, _sz, _sz, _vp, _vp, _vp, _vp]),
	"rk_sdeepenb_set": (_i, [_vp, _i]),
	"rk_sdeepenb_frontiers": (_i, [_vp, _vp, _vp]),
	"rk_sdeepenb_probe": (_i, [_vp, _i, _vp, _vp]),
	"rk_sdeepenb_keys": (_i, [_vp, _vp, _vp]),
	"rk_sdeepenb_paths": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
	"rk_egvm_create": (_i, [C.POINTER(_vp), _i, _i, _i]),
	"rk_egvm_destroy": (_i, [_vp]),
	"rk_egvm_net_in": (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_sz)]),
	"rk_egvm_reset": (_i, [_vp, _vp, C.c_longlong, _vp]),
	"rk_egvm_set_draws": (_i, [_vp, _vp, _i, _vp]),
	"rk_egvm_step": (_i, [_vp, _vp, _i, _vp]),
	"rk_egvm_round_end": (_i, [_vp, _vp, _i, _vp]),
	"rk_egvm_status": (_i, [_vp, _vp, _vp]),
	"rk_egvm_records": (_i, [_vp, C.c_longlong, _i, _vp, _vp]),
	"rk_greedy_create": (_i, [C.POINTER(_vp), _i, _i, _i]),
	"rk_greedy_destroy": (_i, [_vp]),
	"rk_greedy_net_in": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_sz)]),
	"rk_greedy_reset": (_i, [_vp, _vp, _i, _i, _vp]),
	"rk_greedy_step": (_i, [_vp, _vp, _i, _vp]),
	"rk_greedy_status": (_i, [_vp, _vp, _vp]),
	"rk_greedy_export": (_i, [_vp, _vp, _vp, _vp, _vp]),
	"rk_beam_create": (_i, [C.POINTER(_vp), _vp, _i, _i, _i]),
	"rk_beam_destroy": (_i, [_vp]),
	"rk_beam_net_in": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_sz)]),
	"rk_beam_reset": (_i, [_vp, _vp, C.c_longlong, _vp]),
	"rk_beam_step": (_i, [_vp, _vp, _i, _vp]),
	"rk_beam_status": (_i, [_vp, _vp, _vp]),
	"rk_beam_export": (_i, [_vp, _i, _vp, _vp, _sz, _vp]),
	"rk_beam_path": (C.c_longlong, [_vp, _vp, _sz, _vp]),
	"rk_beamb_create": (_i, [C.POINTER(_vp), _vp, _i, _i, _i, _i]),
	"rk_beamb_destroy": (_i, [_vp]),
	"rk_beamb_net_in": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_sz)]),
	"rk_beamb_reset": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
	"rk_beamb_rest": (_i, [_vp, _i, _vp, _vp]),
	"rk_beamb_step": (_i, [_vp, _vp, _i, _vp]),
	"rk_beamb_status": (_i, [_vp, _vp, _vp]),
	"rk_beamb_paths": (_i, [_vp, _vp, _i, _vp]),
	"rk_beamb_export": (_i, [_vp, _i, _i, _vp, _vp, _sz, _vp]),
	"rk_astarb_create": (_i, [C.POINTER(_vp), _i, _sz, _i]),
	"rk_astarb_destroy": (_i, [_vp]),
	"rk_astarb_reset": (_i, [_vp, _vp, _vp, C.c_double, _vp]),
	"rk_astarb_set_values_dtype": (_i, [_vp, _i, _vp]),
	"rk_astarb_step_expand": (_i, [_vp, _vp, _i, _vp]),
	"rk_astarb_step_expand_compact": (_i, [_vp, _vp, _i, _vp, _vp]),
	"rk_astarb_step_commit": (_i, [_vp, _vp, _vp]),
	"rk_astarb_status": (_i, [_vp, _vp, _vp]),
	"rk_astarb_export": (_i, [_vp, _i, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
	"rk_astarb_path": (C.c_longlong, [_vp, _i, C.c_longlong, _vp, _sz, _vp]),
	"rk_astar_create_sharded": (_i, [C.POINTER(_vp), _sz, _i, _i, _i]),
	"rk_shard_owner": (_i, [_vp, _i]),
	"rk_astar_shard_block_bytes": (C.c_longlong, [_vp]),
	"rk_astar_shard_gather_len": (C.c_longlong, [_vp]),
	"rk_astar_shard_gather_ptr": (_vp, [_vp]),
	"rk_astar_shard_bind": (_i, [_vp, _vp]),
	"rk_astar_shard_reset": (_i, [_vp, _vp, C.c_double, _vp, _vp]),
	"rk_astar_shard_select": (_i, [_vp, _vp, C.c_double, C.c_double, _vp, _vp]),
	"rk_astar_shard_decision": (_i, [_vp, _vp, _vp]),
	"rk_astar_shard_insert": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
	"rk_astar_shard_new_count": (_i, [_vp, _vp, _vp]),
	"rk_astar_shard_push": (_i, [_vp, _vp, _vp, _vp, _vp]),
	"rk_astar_shard_push_rows": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
	"rk_astar_shard_flush": (_i, [_vp, _vp, _vp]),
	"rk_astar_shard_clear_send": (_i, [_vp, _vp, _i, _i, _vp]),
	"rk_astar_shard_parent": (_i, [_vp, C.c_longlong, _vp, _vp]),
	"rk_astar_shard_export_ranks": (_i, [_vp, _sz, _sz, _vp, _vp]),
	"rk_comm_unique_id": (_i, [_vp]),
	"rk_comm_create": (_i, [C.POINTER(_vp), _vp, _i, _i]),
	"rk_comm_destroy": (_i, [_vp]),
	"rk_comm_rank": (_i, [_vp]),
	"rk_comm_world": (_i, [_vp]),
	"rk_comm_all_gather": (_i, [_vp, _vp, _vp, _sz, _vp]),
	"rk_comm_all_to_all": (_i, [_vp, _vp, _vp, _sz, _vp]),
	"rk_comm_broadcast": (_i, [_vp, _vp, _sz, _i, _vp]),
	"rk_mcts_create": (_i, [C.POINTER(_vp), _i, _sz, _sz]),
	"rk_mcts_destroy": (_i, [_vp]),
	"rk_mcts_reset": (_i, [_vp, _vp, _vp, C.c_double, C.c_double, _vp]),
	"rk_mcts_roots_oh": (_i, [_vp, _vp, _i, _vp]),
	"rk_mcts_set_root_pv": (_i, [_vp, _vp, _vp, _vp]),
	"rk_mcts_expand": (_i, [_vp, _vp]),
	"rk_mcts_set_expand_ahead": (_i, [_vp, C.c_longlong]),
	"rk_mcts_children_oh": (_i, [_vp, _vp, _i, _vp]),
	"rk_mcts_backup_select": (_i, [_vp, _vp, _vp, _vp]),
	"rk_mcts_backup_select_logits": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp]),
	"rk_mcts_backup_select_logits_range": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _vp]),
	"rk_mcts_children": (_vp, [_vp]),
	"rk_mcts_status": (_i, [_vp, _vp, _vp]),
	"rk_mcts_export": (_i, [_vp, _i, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
	"rk_mcts_path": (C.c_longlong, [_vp, _i, _vp, _vp, _sz, _vp]),
	"rk_mcts_grow": (_i, [_vp, _sz, _sz, _vp, _vp]),
	"rk_mcts_search_graph": (_i, [_vp, _vp]),
	"rk_mcts_graph_path": (C.c_longlong, [_vp, _i, _vp, _sz, _vp]),
	"rk_multi_rotate_host": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
	"rk_expand12_host": (_i, [_i, _vp, _vp, _vp, _vp, _sz, _vp]),
	"rk_multi_is_solved_host": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
	"rk_apply_sequences_host": (_i, [_i, _vp, _i, _i, _i, _i, _vp, _vp]),
	"rk_as_oh_host": (_i, [_i, _vp, _vp, _i, _sz, _vp]),
	"rk_oh686_from2024_host": (_i, [_vp, _vp, _i, _sz, _vp]),
	"rk_686_to2024_host": (_i, [_vp, _vp, _vp, _sz, _vp]),
}

_lib = None


class RubiksHipError(RuntimeError):
	pass


def lib():
	"""The loaded library.  Raises ImportError when it has not been built (python -m librubiks_amd.build)."""
	global _lib
	if _lib is None:
		if not os.path.exists(LIB_PATH):
			raise ImportError(
				f"{LIB_PATH} is missing: build it with `python -m librubiks_amd.build` (hipcc, gfx950). "
				"librubiks_amd has no CPU fallback.")
		handle = C.CDLL(LIB_PATH)
		for name, (res, args) in SIGNATURES.items():
			fn = getattr(handle, name)
			fn.restype, fn.argtypes = res, args
		_lib = handle
	return _lib


def check(rc: int):
	if rc != 0:
		raise RubiksHipError(f"librubiks_hip error {rc}: {lib().rk_last_error().decode()}")


class Owner:
	"""
	Owns one object of the library: made by an `rk_*_create` entry point, destroyed by its `rk_*_destroy` exactly once.  `_h` is
	the handle the other entry points take, None while there is no object (before the first `_create`, after `_free`).
	"""
	_h = None
	_destroy = None

	def _create(self, create: str, destroy: str, *args):
		self._free()
		h = C.c_void_p()
		check(getattr(lib(), create)(C.byref(h), *args))
		self._h, self._destroy = h, destroy
		return h

	def _free(self):
		h, self._h = self._h, None
		if h is not None:
			getattr(lib(), self._destroy)(h)

	def __del__(self):
		try:
			self._free()
		except Exception:
			pass


_gpu_seen = False


def require_gpu():
	global _gpu_seen
	if not _gpu_seen:                      # asked once: a device does not disappear, and the question costs a microsecond per launch
		if not torch.cuda.is_available():
			raise RubiksHipError("no HIP device visible: librubiks_amd computes only on a gfx950 GPU (no CPU fallback)")
		_gpu_seen = True


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


_registered_streams = {0}          # the null stream needs no registration


def stream_ptr() -> int:
	"""hipStream_t of torch's current stream, so that kernels order with the caller's torch work.  (The raw accessor skips
	building a torch.cuda.Stream object: a launch through this shim costs the host about 8 us -- profiles/r03_kernels.json,
	"LAUNCH FLOOR" -- and a third of that was this call.)  A stream seen for the first time is registered with the library
	(rk_stream_register): torch's streams come from a pool and are never destroyed, which is what registration promises.  The owner
	of a `torch.cuda.ExternalStream` calls `forget_stream` before destroying it."""
	s = _raw_stream(torch.cuda.current_device()) if _raw_stream is not None else torch.cuda.current_stream().cuda_stream
	if s not in _registered_streams:
		lib().rk_stream_register(s)
		_registered_streams.add(s)
	return s


def forget_stream(stream) -> None:
	"""Before a stream that was current during a call into this package is destroyed (only external streams ever are)."""
	s = int(getattr(stream, "cuda_stream", stream) or 0)
	if s:
		lib().rk_stream_forget(s)
		_registered_streams.discard(s)
