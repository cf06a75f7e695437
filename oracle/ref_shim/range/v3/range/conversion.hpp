// Stand-in for range-v3 0.11.0's range/conversion.hpp: the reference headers include it but use nothing from it.
#pragma once
