// pcp::traits::is_point -- what surface_nets asks of its vertex type (include/pcp/traits/point_traits.hpp of the
// reference, reduced to what this library uses): x(), y(), z() and construction from three coordinates.
#ifndef PCP_TRAITS_POINT_TRAITS_HPP
#define PCP_TRAITS_POINT_TRAITS_HPP

#include <type_traits>
#include <utility>

namespace pcp {
namespace traits {

template <class Point, class = void>
struct is_point : std::false_type
{
};

template <class Point>
struct is_point<
    Point,
    std::void_t<typename Point::coordinate_type, decltype(std::declval<Point const&>().x()), decltype(std::declval<Point const&>().y()),
                decltype(std::declval<Point const&>().z())>>
    : std::bool_constant<std::is_constructible_v<Point, typename Point::coordinate_type, typename Point::coordinate_type,
                                                 typename Point::coordinate_type>>
{
};

template <class Point>
static constexpr bool is_point_v = is_point<Point>::value;

} // namespace traits
} // namespace pcp

#endif
