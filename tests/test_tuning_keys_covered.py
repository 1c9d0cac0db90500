"""Ledger of the option and tuning keys of libjrx_hip (the two key tables of csrc/handle.hip) against the tests that select a non-default value of each.

include/jrx_tuning.h promises that results never depend on a switch; that promise is only as good as the parity test under every switch.  This file keeps the gap
closed without a GPU: a key added to the table has to be entered here, either with the test functions that run a non-default value of it (each must exist, and its
source -- the function with its decorators, a helper of its module that it calls, or a module-level table it names, such as PIPELINES in test_gpu_two_blocks.py -- must
name the key as a whole word, quoted or as a keyword) or with
one of two exemptions: the key selects no kernel form, or it is a read-only counter."""
import ast
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
TESTS = ROOT / "tests"
NOT_A_FORM = "not a kernel form"
READ_ONLY = "read-only"

# key -> list of "file.py::test function" | (exemption, why)
LEDGER = {
    # ---- options of the public ABI (include/jrx.h)
    "kernel_variant": ["test_gpu_stokes3d.py::test_kernel_variants_are_bit_identical", "test_gpu_stokes2d_thermal.py::test_2d_fused_iteration_with_batched_loads_is_bit_identical"],
    "fused_overlap": ["test_gpu_two_blocks.py::test_two_blocks_equal_the_undecomposed_run_bit_for_bit",
                      "test_gpu_two_blocks.py::test_two_blocks_in_the_viscous_limit_equal_the_undecomposed_general_kernels"],
    "thermal_fused": ["test_gpu_thermal3d.py::test_tiled_fused_iteration_keeps_the_bits", "test_gpu_thermal_multiphase.py::test_fused_3d_phase_form_in_graphs_equals_plain_launches_and_the_two_kernels"],
    "fused_comm": ["test_gpu_two_blocks.py::test_two_blocks_equal_the_undecomposed_run_bit_for_bit"],
    "loop_graphs": ["test_gpu_small_grid_graphs.py::test_stokes3d_graph_replay_changes_nothing", "test_gpu_small_grid_graphs.py::test_vep3d_graph_replay_changes_nothing",
                    "test_gpu_small_grid_graphs.py::test_thermal3d_graph_replay_changes_nothing"],
    "scratch_sets": ["test_gpu_stokes3d.py::test_without_a_second_state_set_the_sweeps_run_and_the_bits_stay"],
    "viscous_limit": ["test_gpu_stokes3d.py::test_viscous_limit_kernel_equals_the_general_one"],
    "field_placement": ["test_gpu_field_alloc.py::test_solve_on_library_arrays_gives_the_same_bits", "test_gpu_two_blocks.py::test_two_blocks_on_pool_placed_library_arrays_keep_the_bits"],
    "field_chunk_mib": ["test_gpu_field_alloc.py::test_solve_on_library_arrays_gives_the_same_bits", "test_gpu_two_blocks.py::test_two_blocks_on_pool_placed_library_arrays_keep_the_bits"],
    "operand_cache": ["test_gpu_stokes3d.py::test_operand_cache_reuses_the_verdict_until_the_fields_are_declared_dirty"],
    # ---- tuning switches (include/jrx_tuning.h)
    "fused_split": ["test_gpu_stokes3d.py::test_every_switch_selected_form_of_the_fused_kernel_keeps_the_bits",
                    "test_gpu_two_blocks.py::test_two_blocks_in_the_viscous_limit_equal_the_undecomposed_general_kernels"],
    "fused_tile": ["test_gpu_stokes3d.py::test_kernel_variants_are_bit_identical", "test_gpu_stokes3d.py::test_viscous_limit_kernel_equals_the_general_one",
                   "test_gpu_stokes3d.py::test_every_switch_selected_form_of_the_fused_kernel_keeps_the_bits"],
    "fused_ylds": ["test_gpu_stokes3d.py::test_every_switch_selected_form_of_the_fused_kernel_keeps_the_bits"],
    "fused_hiface": ["test_gpu_stokes3d.py::test_every_switch_selected_form_of_the_fused_kernel_keeps_the_bits"],
    "visc_fold": ["test_gpu_stokes3d.py::test_every_switch_selected_form_of_the_fused_kernel_keeps_the_bits"],
    "zero_forces": ["test_gpu_stokes3d.py::test_body_forces_that_are_zero_are_not_loaded_and_the_bits_stay",
                    "test_gpu_vep3d.py::test_vep3d_velocity_sweep_does_not_load_body_forces_that_are_zero"],
    "scratch_stagger": (NOT_A_FORM, "where the second state set starts inside its allocation"),
    "scratch_contiguous": (NOT_A_FORM, "the physical backing of the second state set"),
    "end_flips": ["test_gpu_stokes3d.py::test_iterate_timed_with_an_odd_number_of_fused_steps_ends_in_the_user_arrays_without_a_copy"],
    "comm_bcs_lazy": ["test_gpu_two_blocks.py::test_two_blocks_equal_the_undecomposed_run_bit_for_bit"],
    "fused_first_pct": ["test_gpu_two_blocks.py::test_two_blocks_in_the_viscous_limit_equal_the_undecomposed_general_kernels"],
    "b_width_x": ["test_gpu_two_blocks.py::test_two_blocks_equal_the_undecomposed_run_bit_for_bit"],
    "b_width_y": ["test_gpu_two_blocks.py::test_two_blocks_equal_the_undecomposed_run_bit_for_bit"],
    "b_width_z": ["test_gpu_two_blocks.py::test_two_blocks_equal_the_undecomposed_run_bit_for_bit"],
    "halo_self_rccl": ["test_gpu_halo.py::test_periodic_self_exchange", "test_gpu_halo.py::test_solve_on_the_multi_gpu_path_matches_oracle_with_periodic_halo"],
    "thermal_cfg": ["test_gpu_heat_diffusion_inputs.py::test_heat_diffusion_3d_inputs", "test_gpu_thermal3d.py::test_xcd_bands_of_the_fused_iteration_keep_the_bits"],
    "thermal_xg": ["test_gpu_thermal3d.py::test_xcd_bands_of_the_fused_iteration_keep_the_bits"],
    "thermal_tile": ["test_gpu_thermal3d.py::test_tiled_fused_iteration_keeps_the_bits"],
    "thermal_nt": ["test_gpu_thermal3d.py::test_non_temporal_stores_of_the_fused_iteration_keep_the_bits",
                   "test_gpu_thermal_multiphase.py::test_3d_phase_form_with_a_constant_phase_count_in_every_launch_pipeline"],
    "fused2d": ["test_gpu_small_grid_graphs.py::test_2d_iteration_on_either_side_of_fused2d_max_nodes_keeps_the_bits"],
    "vep3_edges": ["test_gpu_vep3d.py::test_update_stresses_3d_matches_oracle", "test_gpu_vep3d.py::test_update_stresses_3d_edge_kernel_configurations"],
    "vep3_cfg": ["test_gpu_vep3d.py::test_update_stresses_3d_edge_kernel_configurations", "test_gpu_vep3d.py::test_update_stresses_3d_eight_plane_chunks_with_other_phase_counts"],
    "vep3_peel": ["test_gpu_vep3d.py::test_update_stresses_3d_without_the_peel_launch"],
    "vep3_nt": ["test_gpu_vep3d.py::test_vep3d_solve_with_non_temporal_stores_keeps_the_bits"],
    "vep3_prekz": ["test_gpu_vep3d.py::test_vep3d_fused_pre_centre_equals_the_three_kernels"],
    "vep3_hide_comm": ["test_gpu_two_blocks.py::test_vep3d_two_blocks_equal_the_undecomposed_run"],
    "vep3_fuse_pc": ["test_gpu_vep3d.py::test_vep3d_fused_pre_centre_equals_the_three_kernels"],
    "vep3_np_const": ["test_gpu_vep3d.py::test_vep3d_solve_with_other_phase_counts_fused_equals_unfused", "test_gpu_vep2d.py::test_vep2d_batched_kernels_equal_the_control_flow_kernels"],
    "vep3_prec_tile": ["test_gpu_vep3d.py::test_vep3d_fused_pre_centre_equals_the_three_kernels"],
    "thermal_np_const": ["test_gpu_thermal_multiphase.py::test_phase_count_constant_kernels_equal_the_run_time_loops"],
    "thermal_fused_ph": ["test_gpu_thermal_multiphase.py::test_3d_phase_form_with_a_constant_phase_count_in_every_launch_pipeline"],
    "fused2d_batch": ["test_gpu_stokes2d_thermal.py::test_2d_fused_iteration_with_batched_loads_is_bit_identical", "test_gpu_vep2d.py::test_vep2d_batched_kernels_equal_the_control_flow_kernels"],
    "fused2d_max_nodes": ["test_gpu_small_grid_graphs.py::test_2d_iteration_on_either_side_of_fused2d_max_nodes_keeps_the_bits"],
    "vep3_map": ["test_gpu_vep3d.py::test_update_stresses_3d_thread_maps_of_the_node_kernel"],
    "vep3_xcd": ["test_gpu_vep3d.py::test_update_stresses_3d_thread_maps_of_the_node_kernel"],
    "comm_timeout_ms": (NOT_A_FORM, "how long a rank waits for a neighbour"),
    "vep_store_all": ["test_gpu_vep3d.py::test_vep3d_solve_that_stores_every_iteration_keeps_the_bits", "test_gpu_vep2d.py::test_vep2d_solve_that_stores_every_iteration_keeps_the_bits",
                      "test_gpu_variational_stokes.py::test_full_solve_that_stores_every_iteration_keeps_the_bits"],
    "chain_profile": (NOT_A_FORM, "event records around the stages of a timed multi-rank step"),
    "general_hif": ["test_gpu_stokes3d.py::test_general_form_folds_its_high_face_layers",
                    "test_gpu_two_blocks.py::test_blocks_with_finite_dt_finish_their_neighbour_faces_inside_the_general_kernel"],
    "field_shuffle": (NOT_A_FORM, "the order in which physical chunks are dealt to arrays"),
    "field_pool_pct": (NOT_A_FORM, "the size of the pool of physical chunks"),
    "fused_kz": ["test_gpu_stokes3d.py::test_chunk_depths_of_the_tall_tile_keep_the_bits"],
    "fused_ym": ["test_gpu_stokes3d.py::test_y_march_of_the_fused_kernel_keeps_the_bits"],
    "nbr_feeder": ["test_gpu_two_blocks.py::test_two_blocks_in_the_viscous_limit_equal_the_undecomposed_general_kernels"],
    "scratch_poison": (NOT_A_FORM, "what library-owned arrays hold before their first use"),
    "weno_fused": ["test_gpu_weno5.py::test_fused_form_is_bit_identical_to_the_per_kernel_form", "test_gpu_weno5_3d.py::test_fused_form_is_bit_identical_to_the_per_kernel_form"],
    "weno_rows": ["test_gpu_weno5.py::test_fused_form_is_bit_identical_to_the_per_kernel_form", "test_gpu_weno5_3d.py::test_fused_form_is_bit_identical_to_the_per_kernel_form"],
    "phase_ratios_fused": ["test_gpu_phase_ratios.py::test_both_forms_leave_identical_bits"],
    "rock_fraction3d_rows": ["test_gpu_topography3d.py::test_rock_fraction_equals_the_restatement_bit_for_bit"],
    "particles_stress_fused": ["test_gpu_particles2d_stress.py::test_rotate_stress_one_launch_equals_its_chain_and_the_restatement", "test_gpu_particles2d_stress.py::test_stress2grid_one_launch_equals_its_chain_and_the_restatement"],
    "particles_subgrid_fused": ["test_gpu_particles2d_subgrid.py::test_the_fused_form_equals_its_chain_and_the_restatement"],
    "particles3d_move_codes": ["test_gpu_particles3d.py::test_a_rigid_rotation_at_courant_half_advects_and_moves_bit_for_bit"],
    "particles3d_ratios_split": ["test_gpu_particles3d.py::test_phase_ratios_bit_for_bit_with_an_emptied_cell"],
}
# what a test may write instead of the key itself: the keyword of the package's wrapper that sets it
ALIASES = {"halo_self_rccl": "self_rccl"}
EXEMPT_NOT_A_FORM = {"scratch_stagger", "scratch_contiguous", "comm_timeout_ms", "chain_profile", "field_shuffle", "field_pool_pct", "scratch_poison"}


def table_keys():
    """(key, kind) of every entry of the two OptRef tables of find_opt (kind 0: bool, 1: int, 2: read-only counter)"""
    src = (ROOT / "justrelax.jl_amd" / "csrc" / "handle.hip").read_text()
    body = src[src.index("int find_opt("):src.index("jrx_status opt_set(")]
    return [(m.group(1), int(m.group(2))) for m in re.finditer(r'\{"([A-Za-z0-9_]+)",\s*([012]),\s*&h->', body)]


def names(key, src):
    """the key as a whole word -- "fused2d" is not named by "fused2d_batch" or "stat_fused2d" -- written the way a key is handed to the library: a quoted string or a keyword (key=...)"""
    k = re.escape(key)
    return re.search(r"""["']%s["']|(?<![A-Za-z0-9_])%s\s*=(?!=)""" % (k, k), src) is not None


class Module:
    """the test functions of one file and its module-level tables, as source text"""
    _cache = {}

    def __new__(cls, name):
        if name not in cls._cache:
            self = super().__new__(cls)
            text = (TESTS / name).read_text()
            tree = ast.parse(text)
            lines = text.splitlines()
            self.functions, self.tables = {}, {}
            for node in tree.body:
                if isinstance(node, ast.FunctionDef):
                    first = min([node.lineno] + [d.lineno for d in node.decorator_list])
                    self.functions[node.name] = "\n".join(lines[first - 1:node.end_lineno])
                elif isinstance(node, ast.Assign):
                    for t in node.targets:
                        if isinstance(t, ast.Name):
                            self.tables[t.id] = "\n".join(lines[node.lineno - 1:node.end_lineno])
            cls._cache[name] = self
        return cls._cache[name]

    def mentions(self, function, word):
        """in the function (decorators included), in a module-level table it names, or in a helper of the module it calls"""
        seen, todo = set(), [function]
        while todo:
            f = todo.pop()
            if f in seen:
                continue
            seen.add(f)
            src = self.functions[f]
            if names(word, src) or any(re.search(r"\b%s\b" % re.escape(t), src) and names(word, s) for t, s in self.tables.items()):
                return True
            todo += [g for g in self.functions if g not in seen and not g.startswith("test_") and re.search(r"\b%s\(" % re.escape(g), src)]
        return False


def test_the_table_has_keys_and_every_counter_is_read_only():
    keys = table_keys()
    assert len(keys) > 60 and len({k for k, _ in keys}) == len(keys)
    for k, kind in keys:
        assert (kind == 2) == k.startswith("stat_"), k


def test_every_key_of_the_table_is_in_the_ledger():
    missing = [k for k, kind in table_keys() if kind != 2 and k not in LEDGER]
    assert not missing, "keys of csrc/handle.hip without a parity test or an exemption in tests/test_tuning_keys_covered.py: %s" % missing
    gone = [k for k in LEDGER if k not in {k for k, _ in table_keys()}]
    assert not gone, "ledger entries for keys that are no longer in the table: %s" % gone


def test_exemptions_are_the_allowed_ones():
    for k, kind in table_keys():
        if kind == 2:
            assert k not in LEDGER or LEDGER[k] == (READ_ONLY, "")       # a counter needs no entry
            continue
        e = LEDGER[k]
        if isinstance(e, tuple):
            assert e[0] == NOT_A_FORM and k in EXEMPT_NOT_A_FORM and e[1], k
        else:
            assert e, k


@pytest.mark.parametrize("key", [k for k, e in LEDGER.items() if isinstance(e, list)])
def test_the_tests_of_a_key_exist_and_mention_it(key):
    word = ALIASES.get(key, key)
    for entry in LEDGER[key]:
        name, _, function = entry.partition("::")
        assert (TESTS / name).exists(), entry
        mod = Module(name)
        assert function.startswith("test_") and function in mod.functions, "%s: no such test function" % entry
        assert mod.mentions(function, word), "%s does not mention '%s'" % (entry, word)
