// gnerf_query_lattice: the densities-only point query at lattice points named by their linear index (query_lattice.inl has the kernel and
// the entry point).  A translation unit of its own: it needs the renderer's generic lookup and decoder (render_core.inl) and the point
// queries' fill_query (query_fill.inl), nothing else of csrc/render_query.hip.
#include "render_core.inl"
#include "query_fill.inl"
#include "query_lattice.inl"
