// graph_pairs.hip — the pair-table form of the minutiae list kernel (afis_correspondences_pairs): k_graph_minutiae<REF_TIE, const int32_t*> and its launcher
// launch_graph_minutiae_pairs, compiled from graph.hip itself in a translation unit of their own (see k_graph_minutiae there).  Built with graph.hip's flags.
// A PHASE_TIMING build compiles this unit WITHOUT the phase timers (their counters are a device variable of graph.hip's module): afis_debug_phase_cycles counts the
// search's list launches only, never the pair launches.
#define AFIS_GRAPH_PAIRS_UNIT
#include "graph.hip"
