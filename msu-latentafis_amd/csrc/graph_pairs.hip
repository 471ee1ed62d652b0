// graph_pairs.hip — the pair-table forms of the list kernels: k_graph_minutiae<REF_TIE, const int32_t*> with its launcher launch_graph_minutiae_pairs
// (afis_correspondences_pairs, afis_score_pairs) and k_graph_texture<REF_TIE, const int32_t*> with launch_graph_texture_pairs (afis_score_pairs; with its tap after S9, the evidence calls of afis_evidence.cpp), compiled from graph.hip
// itself in a translation unit of their own (see k_graph_minutiae there).  Built with graph.hip's flags.
// A PHASE_TIMING build compiles this unit WITHOUT the phase timers (their counters are a device variable of graph.hip's module): afis_debug_phase_cycles counts the
// search's list launches only, never the pair launches.
#define AFIS_GRAPH_PAIRS_UNIT
#include "graph.hip"
