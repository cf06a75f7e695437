// pcp::traits::is_shared_vertex_mesh_triangle -- a triangle that stores three vertex indices
// (include/pcp/traits/triangle_traits.hpp of the reference): index_type, indices(), constructible from three indices.
#ifndef PCP_TRAITS_TRIANGLE_TRAITS_HPP
#define PCP_TRAITS_TRIANGLE_TRAITS_HPP

#include <type_traits>
#include <utility>

namespace pcp {
namespace traits {

template <class SharedVertexMeshTriangle, class = void>
struct is_shared_vertex_mesh_triangle : std::false_type
{
};

template <class SharedVertexMeshTriangle>
struct is_shared_vertex_mesh_triangle<
    SharedVertexMeshTriangle,
    std::void_t<typename SharedVertexMeshTriangle::index_type, decltype(std::declval<SharedVertexMeshTriangle&>().indices())>>
    : std::bool_constant<std::is_constructible_v<
          SharedVertexMeshTriangle,
          typename SharedVertexMeshTriangle::index_type,
          typename SharedVertexMeshTriangle::index_type,
          typename SharedVertexMeshTriangle::index_type>>
{
};

template <class SharedVertexMeshTriangle>
static constexpr bool is_shared_vertex_mesh_triangle_v = is_shared_vertex_mesh_triangle<SharedVertexMeshTriangle>::value;

} // namespace traits
} // namespace pcp

#endif
