from ppsurf_amd.visualization import (render_scene, distances_to_vertex_colors, visualize_chamfer_distance,  # noqa: F401
                                      visualize_chamfer_distance_pool, render_meshes, get_closest_point_on_mesh)
