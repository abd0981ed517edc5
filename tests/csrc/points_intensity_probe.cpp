// Host-only probe for tests/test_points_cpu.py: what g++ makes of the reference's intensity expression
// static_cast<uint8_t>(*iter_intensity_in * 255) (generic_points_input.hpp:46) when the iterator is a PointCloud2ConstIterator<uint8_t>,
// i.e. a const uint8_t* into the message bytes. Prints "<byte> <result>" for the 256 byte values. No HIP, no GPU.
#include <cstdint>
#include <cstdio>

int main()
{
    static uint8_t field[256];
    for (int b = 0; b < 256; b++)
        field[b] = static_cast<uint8_t>(b);
    const volatile uint8_t* it = field; // volatile: computed at run time, as on a message
    for (int b = 0; b < 256; b++, ++it)
    {
        const uint8_t intensity = static_cast<uint8_t>(*it * 255);
        printf("%d %d\n", b, static_cast<int>(intensity));
    }
    return 0;
}
