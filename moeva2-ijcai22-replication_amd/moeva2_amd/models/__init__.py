"""Model descriptions the engine runs on the device besides the Dense MLP."""
