/* Stand-in for the HDK's UT_Interrupt: never interrupted.  See SYS/SYS_Types.h. */
#ifndef REFSTANDIN_UT_INTERRUPT_H
#define REFSTANDIN_UT_INTERRUPT_H

class UT_Interrupt
{
public:
    bool opInterrupt(int = -1) { return false; }
};

inline UT_Interrupt *UTgetInterrupt()
{
    static UT_Interrupt boss;
    return &boss;
}

#endif
