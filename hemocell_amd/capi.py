"""ctypes binding of hemocell_amd/lib/libhemocell_amd.so (the C ABI declared in
include/hemocell_amd.h).  No compute happens in Python; if the HIP library is
missing or no gfx950 device is usable every call raises -- there is no CPU
fallback in the product path."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhemocell_amd.so")

c_double_p = C.POINTER(C.c_double)
c_long_p = C.POINTER(C.c_long)
c_int_p = C.POINTER(C.c_int)


class HcError(RuntimeError):
    pass


class Params(C.Structure):
    """hc_params == Parameters::lbm_base_parameters (mechanics/constantConversion.cpp:36-59)"""
    _fields_ = [(n, C.c_double) for n in
                ("dx", "dt", "nu_p", "rho_p", "kBT_p", "tau", "nu_lbm", "dm", "df", "f_limit", "kBT_lbm")]


class Material(C.Structure):
    """hc_material == <MaterialModel> of RBC.xml / PLT.xml"""
    _fields_ = [("kLink", C.c_double), ("kArea", C.c_double), ("kVolume", C.c_double), ("kBend", C.c_double),
                ("eta_m", C.c_double), ("radius", C.c_double), ("min_triangles", C.c_int),
                ("aspect_ratio", C.c_double), ("inner_edges", c_long_p), ("n_inner", C.c_int)]


class WbcMaterial(C.Structure):
    """hc_wbc_material == the extra <MaterialModel> tags of WBC_HO.xml (SI units)"""
    _fields_ = [("kInnerRigid", C.c_double), ("kCytoskeleton", C.c_double), ("coreRadius", C.c_double),
                ("radius", C.c_double)]


class CellTypeSpec(C.Structure):
    """hc_celltype_spec == everything addCellType<Model>(name, constructType) reads from a cell XML"""
    _fields_ = [("model", C.c_int), ("shape", C.c_int), ("material", Material), ("wbc", C.POINTER(WbcMaterial)),
                ("kInnerLink", C.c_double), ("stl_path", C.c_char_p)]


# every symbol include/hemocell_amd.h declares: name -> (restype, argtypes)
VP = C.c_void_p
SIGNATURES = {
    "hc_last_error": (C.c_char_p, []),
    "hc_init": (C.c_int, [C.c_int]),
    "hc_device_count": (C.c_int, [c_int_p]),
    "hc_set_stream": (C.c_int, [VP]),
    "hc_synchronize": (C.c_int, []),
    "hc_fork": (C.c_int, []),
    "hc_route": (C.c_int, [C.c_int]),
    "hc_join": (C.c_int, []),
    "hc_side_stream": (C.c_int, [C.POINTER(VP)]),
    "hc_set_overlap": (C.c_int, [C.c_int]),
    "hc_comm_init_env": (C.c_int, []),
    "hc_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int]),
    "hc_comm_finalize": (C.c_int, []),
    "hc_comm_info": (C.c_int, [c_int_p, c_int_p, c_int_p]),
    "hc_comm_barrier": (C.c_int, []),
    "hc_comm_allreduce": (C.c_int, [c_double_p, C.c_int, C.c_int]),
    "hc_comm_bcast": (C.c_int, [VP, C.c_size_t, C.c_int]),
    "hc_comm_allgather": (C.c_int, [VP, C.c_size_t, VP]),
    "hc_comm_exchange_host": (C.c_int, [C.c_int, VP, C.c_size_t, VP, C.c_size_t, VP, C.c_size_t, VP, C.c_size_t]),
    "hc_slab_stats": (C.c_int, [VP, c_double_p, C.c_int]),
    "hcl_slab_refresh_halos": (C.c_int, [VP, C.c_int]),
    "hcp_slab_sync_placement": (C.c_int, [VP, c_long_p]),
    "hcp_set_envelope": (C.c_int, [VP, C.c_double, c_double_p]),
    "hcp_envelope": (C.c_int, [VP, c_double_p, c_long_p]),
    "hcp_set_deletion_mode": (C.c_int, [VP, C.c_int]),
    "hcp_delete_incomplete_cells": (C.c_int, [VP, c_long_p]),
    "hcp_deletion_counts": (C.c_int, [VP, c_long_p, c_long_p, c_long_p, c_long_p]),
    "hcp_download_alive": (C.c_int, [VP, VP]),
    "hc_profile_enable": (C.c_int, [C.c_int]),
    "hc_profile_read": (C.c_int, [C.c_char_p, c_double_p, c_long_p]),
    "hc_profile_reset": (C.c_int, []),
    "hc_build_tag": (C.c_char_p, []),
    "hc_measure_copy_bandwidth": (C.c_int, [C.c_size_t, C.c_int, c_double_p]),
    "hcl_node_counts": (C.c_int, [VP, c_long_p]),
    "hc_debug_ibm_per_vertex": (C.c_int, [C.c_int]),
    "hc_set_reproducible_spread": (C.c_int, [C.c_int]),
    "hc_debug_force_plane_padding": (C.c_int, [C.c_int]),
    "hcl_create": (C.c_int, [C.POINTER(VP), C.c_int, C.c_int, C.c_int, c_int_p, C.c_double, C.c_int, C.c_int, C.c_int]),
    "hcl_destroy": (C.c_int, [VP]),
    "hcl_set_mask": (C.c_int, [VP, VP]),
    "hcl_init_equilibrium": (C.c_int, [VP, C.c_double, c_double_p]),
    "hcl_set_body_force_regions": (C.c_int, [VP, C.c_int, C.POINTER(C.c_int), c_double_p]),
    "hcl_set_body_force": (C.c_int, [VP, c_double_p]),
    "hcl_set_wall_velocity": (C.c_int, [VP, C.c_int, c_double_p]),
    "hcl_collide_stream": (C.c_int, [VP, C.c_int]),
    "hcl_set_lees_edwards": (C.c_int, [VP, C.c_double, C.c_double]),
    "hcl_set_lees_edwards_displacement": (C.c_int, [VP, C.c_double, C.c_double]),
    "hcl_lees_edwards_apply": (C.c_int, [VP]),
    "hcl_lees_edwards_state": (C.c_int, [VP, c_double_p]),
    "hcl_open_boundary_add": (C.c_int, [VP, C.c_int, C.c_int, c_int_p, C.c_int, c_int_p]),
    "hcl_open_boundary_add_box": (C.c_int, [VP, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p]),
    "hcl_open_boundary_add_axis": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, c_int_p, C.c_int, c_int_p]),
    "hcl_open_boundary_add_box_axis": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p]),
    "hcl_open_boundary_axes": (C.c_int, [VP, c_int_p, C.c_int, c_int_p]),
    "hcl_open_boundary_clear": (C.c_int, [VP]),
    "hcl_open_boundary_slots": (C.c_int, [VP, c_int_p, C.c_int, c_int_p]),
    "hcl_open_boundary_set_velocity": (C.c_int, [VP, C.c_int, C.c_int, VP, C.c_int]),
    "hcl_open_boundary_set_density": (C.c_int, [VP, C.c_int, C.c_int, VP, C.c_int]),
    "hcl_open_boundary_values": (C.c_int, [VP, C.c_int, C.c_int, c_double_p]),
    "hcl_plane_velocity": (C.c_int, [VP, C.c_int, c_int_p, C.c_int, VP, C.c_int]),
    "hcl_plane_velocity_axis": (C.c_int, [VP, C.c_int, C.c_int, c_int_p, C.c_int, VP, C.c_int]),
    "hcl_preinlet_create": (C.c_int, [C.POINTER(VP), VP, VP, C.c_int, C.c_int, c_int_p, C.c_int, C.c_int]),
    "hcl_preinlet_apply": (C.c_int, [VP]),
    "hcl_preinlet_iterate": (C.c_int, [VP, C.c_int]),
    "hcl_preinlet_destroy": (C.c_int, [VP]),
    "hcl_collide_stream_part": (C.c_int, [VP, C.c_int]),
    "hcl_step_end": (C.c_int, [VP]),
    "hcl_download_populations": (C.c_int, [VP, c_double_p]),
    "hcl_upload_populations": (C.c_int, [VP, c_double_p]),
    "hcl_download_rho_u": (C.c_int, [VP, c_double_p, c_double_p]),
    "hcl_download_pi_neq": (C.c_int, [VP, c_double_p]),
    "hcl_download_ibm_force": (C.c_int, [VP, c_double_p]),
    "hcl_zero_ibm_force": (C.c_int, [VP]),
    "hcl_halo_doubles": (C.c_size_t, [VP, C.c_int]),
    "hcl_halo_pack": (C.c_int, [VP, C.c_int, C.c_int, VP]),
    "hcl_halo_unpack": (C.c_int, [VP, C.c_int, C.c_int, VP]),
    "hcl_halo_pack_next": (C.c_int, [VP, C.c_int, C.c_int, VP]),
    "hcl_face_velocity_pack": (C.c_int, [VP, C.c_int, VP]),
    "hcl_face_velocity_pack_both": (C.c_int, [VP, VP, VP]),
    "hcl_halo_pack_both": (C.c_int, [VP, VP, VP, C.c_int]),
    "hcl_halo_unpack_both": (C.c_int, [VP, VP, VP]),
    "hcl_zero_force_halos": (C.c_int, [VP]),
    "hcl_download_face_velocity": (C.c_int, [VP, C.c_int, c_double_p]),
    "hcl_dims": (C.c_int, [VP, c_int_p]),
    "hcl_mlups_bytes_per_node": (C.c_double, [VP]),
    "hcl_interior_enable": (C.c_int, [VP, C.c_int, c_double_p]),
    "hcl_interior_info": (C.c_int, [VP, c_int_p, c_double_p]),
    "hcl_interior_upload_classes": (C.c_int, [VP, VP]),
    "hcl_interior_download_classes": (C.c_int, [VP, VP]),
    "hcl_scalar_create": (C.c_int, [VP, C.c_double, C.POINTER(VP)]),
    "hcl_scalar_destroy": (C.c_int, [VP]),
    "hcl_scalar_init_equilibrium": (C.c_int, [VP, c_int_p, C.c_double]),
    "hcl_scalar_set_source_box": (C.c_int, [VP, c_int_p, C.c_double]),
    "hcl_scalar_clear_sources": (C.c_int, [VP]),
    "hcl_scalar_step": (C.c_int, [VP]),
    "hcl_scalar_download": (C.c_int, [VP, c_double_p]),
    "hcl_scalar_download_populations": (C.c_int, [VP, c_double_p]),
    "hcl_scalar_upload_populations": (C.c_int, [VP, c_double_p]),
    "hcl_scalar_download_velocity": (C.c_int, [VP, c_double_p]),
    "hcl_scalar_stats": (C.c_int, [VP, c_double_p]),
    "hcp_sample_scalar": (C.c_int, [VP, VP, c_double_p]),
    "hcp_type_set_ibm_kernel": (C.c_int, [VP, C.c_int, C.c_int]),
    "hcp_type_get_ibm_kernel": (C.c_int, [VP, C.c_int, c_int_p]),
    "hcp_type_set_interior_viscosity": (C.c_int, [VP, C.c_int, C.c_double]),
    "hcp_set_interior_timescales": (C.c_int, [VP, C.c_int, C.c_int]),
    "hcp_interior_find": (C.c_int, [VP]),
    "hcp_interior_membrane": (C.c_int, [VP]),
    "hcp_interior_normals": (C.c_int, [VP, C.c_int, c_double_p]),
    "hc_debug_interior_block": (C.c_int, [C.c_int]),
    "hcl_binding_populate": (C.c_int, [VP, c_int_p]),
    "hcl_binding_clear": (C.c_int, [VP]),
    "hcl_binding_download": (C.c_int, [VP, VP]),
    "hcl_binding_upload": (C.c_int, [VP, VP]),
    "hcl_download_mask": (C.c_int, [VP, VP]),
    "hcl_download_tresca": (C.c_int, [VP, c_double_p]),
    "hcl_upload_solidified_mask": (C.c_int, [VP, VP]),
    "hcp_type_set_solidify": (C.c_int, [VP, C.c_int, C.c_double, C.c_double]),
    "hcp_set_solidify_timescale": (C.c_int, [VP, C.c_int]),
    "hcp_solidify_prepare": (C.c_int, [VP]),
    "hcp_solidify_flag": (C.c_int, [VP]),
    "hcp_solidify_flags_download": (C.c_int, [VP, VP]),
    "hcp_solidify_flags_upload": (C.c_int, [VP, VP]),
    "hcp_solidify_counts": (C.c_int, [VP, c_long_p]),
    "hc_debug_solidify_block": (C.c_int, [C.c_int]),
    "hc_params_base": (C.c_int, [C.POINTER(Params)] + [C.c_double] * 5),
    "hcp_celltype_create": (C.c_int, [C.POINTER(VP), C.c_int, C.c_int, C.POINTER(Params), C.POINTER(Material)]),
    "hcp_celltype_create_wbc": (C.c_int, [C.POINTER(VP), C.c_int, C.POINTER(Params), C.POINTER(Material),
                                          C.POINTER(WbcMaterial)]),
    "hcp_celltype_wbc_constants": (C.c_int, [VP, c_double_p]),
    "hcp_celltype_create_ex": (C.c_int, [C.POINTER(VP), C.POINTER(Params), C.POINTER(CellTypeSpec)]),
    "hcp_celltype_malaria_constants": (C.c_int, [VP, c_double_p]),
    "hcp_celltype_destroy": (C.c_int, [VP]),
    "hcp_celltype_sizes": (C.c_int, [VP, c_int_p]),
    "hcp_celltype_tables": (C.c_int, [VP, c_double_p, c_long_p, c_long_p, c_double_p, c_double_p, c_double_p,
                                      c_long_p, c_double_p, c_double_p]),
    "hcp_celltype_tables2": (C.c_int, [VP, c_long_p, c_long_p, c_long_p, c_double_p, c_int_p]),
    "hcp_create": (C.c_int, [C.POINTER(VP), VP, C.POINTER(Params)]),
    "hcp_destroy": (C.c_int, [VP]),
    "hcp_add_type": (C.c_int, [VP, VP, C.c_int, c_int_p]),
    "hcp_add_cell": (C.c_int, [VP, C.c_int, C.c_long, c_double_p, c_double_p, C.c_double, c_int_p]),
    "hcp_add_cell_unchecked": (C.c_int, [VP, C.c_int, C.c_long, c_double_p, c_double_p]),
    "hcp_counts": (C.c_int, [VP, c_long_p, c_long_p, c_long_p]),
    "hcp_type_range": (C.c_int, [VP, C.c_int, c_long_p, c_long_p]),
    "hcp_download": (C.c_int, [VP, C.c_int, c_double_p]),
    "hcp_upload": (C.c_int, [VP, C.c_int, c_double_p]),
    "hcp_download_cell_ids": (C.c_int, [VP, c_long_p]),
    "hcp_download_records": (C.c_int, [VP, C.c_void_p, C.c_long]),
    "hcp_upload_records": (C.c_int, [VP, C.c_void_p, C.c_long]),
    "hcp_add_vertex_force": (C.c_int, [VP, c_long_p, C.c_int, c_double_p]),
    "hcp_set_repulsion": (C.c_int, [VP, C.c_double, C.c_double, C.c_int]),
    "hcp_repulsion": (C.c_int, [VP]),
    "hcp_download_repulsion": (C.c_int, [VP, c_double_p]),
    "hcl_fluid_stats": (C.c_int, [VP, C.c_int, c_double_p, C.POINTER(C.c_long)]),
    "hcp_vertex_stats": (C.c_int, [VP, C.c_int, c_double_p, C.POINTER(C.c_long)]),
    "hcp_set_boundary_repulsion": (C.c_int, [VP, C.c_double, C.c_double, C.c_int]),
    "hcp_boundary_repulsion": (C.c_int, [VP]),
    "hcp_spread": (C.c_int, [VP, C.c_int]),
    "hcp_interpolate": (C.c_int, [VP]),
    "hcp_interpolate_cells": (C.c_int, [VP, C.c_int, c_int_p, C.c_int]),
    "hcp_advance": (C.c_int, [VP, C.c_int]),
    "hcp_mechanics": (C.c_int, [VP, C.c_long, C.c_int]),
    "hcp_mechanics_components": (C.c_int, [VP, C.c_int, c_double_p]),
    "hc_iterate": (C.c_int, [VP, VP, c_long_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hcp_cell_extents": (C.c_int, [VP, C.c_int, c_double_p]),
    "hcp_cell_extents_begin": (C.c_int, [VP, C.c_int]),
    "hcp_cell_extents_end": (C.c_int, [VP, C.c_int, c_double_p]),
    "hcp_record_doubles": (C.c_size_t, [VP, C.c_int]),
    "hcp_pack_cells": (C.c_int, [VP, C.c_int, c_int_p, C.c_int, C.c_double, VP]),
    "hcp_unpack_cells": (C.c_int, [VP, C.c_int, c_int_p, c_long_p, c_int_p, C.c_int, VP]),
    "hcp_remove_cells": (C.c_int, [VP, C.c_int, c_int_p, C.c_int]),
    "hcp_owned_vertices": (C.c_int, [VP, c_long_p]),
    "hcp_preinlet_create": (C.c_int, [C.POINTER(VP), VP, VP, C.c_int, C.c_int, C.c_double, C.c_double, c_double_p, C.c_long]),
    "hcp_preinlet_create_slab": (C.c_int, [C.POINTER(VP), VP, VP, C.c_int, C.c_int, C.c_double, C.c_double, c_double_p, C.c_long]),
    "hcp_preinlet_set_sink": (C.c_int, [VP, C.c_int, C.c_double]),
    "hcp_preinlet_apply": (C.c_int, [VP, c_long_p, c_long_p]),
    "hcp_preinlet_counts": (C.c_int, [VP, c_long_p]),
    "hcp_preinlet_destroy": (C.c_int, [VP]),
    "hc_preinlet_iterate": (C.c_int, [VP, VP, c_long_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hcp_cell_info": (C.c_int, [VP, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_packing_create": (C.c_int, [C.POINTER(VP), c_int_p, C.c_int, c_double_p, c_int_p, c_double_p, c_double_p, C.c_double, C.c_int,
                                    C.c_int, C.c_double]),
    "hc_packing_run": (C.c_int, [VP, C.c_int, c_double_p]),
    "hc_packing_count": (C.c_int, [VP, c_int_p, c_int_p]),
    "hc_packing_state": (C.c_int, [VP, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_packing_pairs": (C.c_int, [C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int, c_double_p,
                                   c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]),
    "hc_packing_destroy": (C.c_int, [VP]),
    "hc_packing_set_walls": (C.c_int, [VP, VP, c_int_p, C.c_double, c_int_p, C.c_double]),
    "hc_packing_wall_field": (C.c_int, [VP, c_double_p]),
    "hc_packing_reserve_lists": (C.c_int, [VP, C.c_int]),
    "hc_packing_walls": (C.c_int, [C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int, c_double_p, c_double_p,
                                   c_double_p, c_int_p, c_int_p]),
    "hc_stats_create": (C.c_int, [VP, VP, C.c_int, C.POINTER(VP)]),
    "hc_stats_destroy": (C.c_int, [VP]),
    "hc_stats_set_every": (C.c_int, [VP, C.c_int]),
    "hc_stats_sample": (C.c_int, [VP]),
    "hc_stats_reset": (C.c_int, [VP]),
    "hc_stats_samples": (C.c_int, [VP, c_long_p]),
    "hc_stats_download_fluid": (C.c_int, [VP, C.c_int, c_double_p]),
    "hc_stats_download_cells": (C.c_int, [VP, C.c_int, C.c_int, c_long_p]),
}

_lib = None


def build():
    """Compile the HIP library in-tree with the committed Makefile."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])


def lib():
    """Load the shared library and bind every declared symbol."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HcError("libhemocell_amd.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                          "the product path has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise HcError(lib().hc_last_error().decode("utf-8", "replace"))


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def lptr(a):
    return a.ctypes.data_as(c_long_p)
