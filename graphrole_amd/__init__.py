"""
graphrole_amd -- MI355X-native ReFeX / RolX engine, drop-in for GraphRole's
``RecursiveFeatureExtractor`` and ``RoleExtractor`` (reference: graphrole/__init__.py:1-2).
"""
__version__ = '0.1.0'


def __getattr__(name):
    # lazy: importing the package must not require a GPU (CPU-side tests import sub-modules)
    if name == 'RecursiveFeatureExtractor':
        from .features.extract import RecursiveFeatureExtractor
        return RecursiveFeatureExtractor
    if name == 'RoleExtractor':
        from .roles.extract import RoleExtractor
        return RoleExtractor
    if name in ('node_measures', 'betweenness_centrality', 'closeness_centrality', 'harmonic_centrality',
                'biconnected_component_counts', 'articulation_points', 'biconnected_components', 'core_number',
                'onion_layers', 'eccentricity', 'diameter', 'radius', 'center', 'periphery', 'constraint',
                'effective_size', 'dijkstra_path_lengths', 'weighted_betweenness_centrality', 'clustering',
                'average_clustering', 'square_clustering', 'truss_number', 'node_truss_number', 'k_truss',
                'graphlet_degree_vectors', 'graphlet_counts', 'neighbor_roles', 'role_mixing_matrix',
                'edge_betweenness_centrality', 'triadic_census', 'node_triad_census', 'ConvergenceError'):
        from . import measures
        return getattr(measures, name)
    if name == 'nearest_nodes':
        from .similarity import nearest_nodes
        return nearest_nodes
    if name in ('connected_components', 'weakly_connected_components', 'strongly_connected_components',
                'number_connected_components', 'number_weakly_connected_components',
                'number_strongly_connected_components', 'is_connected', 'is_weakly_connected', 'is_strongly_connected',
                'component_table', 'largest_component', 'descendants', 'ancestors', 'bow_tie'):
        from . import components
        return getattr(components, name)
    raise AttributeError(name)
